"""Build-time check of the fused P2P update (csrc/cgx_p2p.hip): its four instantiations compile for gfx950 without scratch, and
the production forms stay within their register budgets.  The fused exchange needs every workgroup of its grid resident at
once (the workgroups wait for each other inside the kernel), so more VGPRs would lower the occupancy the host's co-residency
check relies on.  k_update_xr (csrc/cgx_kernels.hip) is the one-GPU K3."""
import os

import pytest

from test_kernel_resources import HIPCC, resources

FORMS = ("<false, false>", "<false, true>", "<true, false>", "<true, true>")   # <TAGGED, SELFTEST>
MAX_VGPRS = {"<false, false>": 58, "<true, false>": 62}                        # the production forms


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_fused_update_instantiations_stay_within_budget():
    rows = {r["name"].split("(")[0]: r for r in resources("cgx_p2p.hip") if "cgx::k_update_xr_p2p" in r["name"]}
    assert sorted(rows) == sorted("void cgx::k_update_xr_p2p" + f for f in FORMS), sorted(rows)
    for name, r in rows.items():
        assert int(r["VGPRs Spill"]) == 0 and int(r["ScratchSize [bytes/lane]"]) == 0, r
    for form, limit in MAX_VGPRS.items():
        assert int(rows["void cgx::k_update_xr_p2p" + form]["VGPRs"]) <= limit, rows["void cgx::k_update_xr_p2p" + form]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_one_gpu_update_keeps_its_registers():
    rows = [r for r in resources("cgx_kernels.hip") if r["name"].startswith("cgx::k_update_xr(")]
    assert len(rows) == 1, [r["name"] for r in rows]
    assert int(rows[0]["VGPRs"]) == 30 and int(rows[0]["ScratchSize [bytes/lane]"]) == 0, rows[0]
