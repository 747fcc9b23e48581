"""Build-time check of the symmetric K1 (csrc/cgx_symv.hip): every kernel instantiation compiles for gfx950 without scratch and
without a vector-register spill, and the tile kernel stays within 128 VGPRs (four workgroups of 256 threads per CU)."""
import os

import pytest

from test_kernel_resources import HIPCC, resources


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_symmetric_kernels_never_spill():
    rows = [r for r in resources("cgx_symv.hip") if "cgx::k_sym" in r["name"]]
    names = sorted(r["name"] for r in rows)
    assert len(rows) == 5, names   # tiles and fold, plain and fused; the symmetry check
    for r in rows:
        assert int(r["VGPRs Spill"]) == 0 and int(r["ScratchSize [bytes/lane]"]) == 0, r
        if "k_symv_tiles" in r["name"]:
            assert int(r["VGPRs"]) <= 128, r
