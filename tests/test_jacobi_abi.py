"""CPU checks of the Jacobi preconditioner (include/cgx.h cgx_set_preconditioner): the C ABI and the Python
constants agree, and a gfx950 cross-compile (`hipcc -Rpass-analysis=kernel-resource-usage`) shows that

  - no Jacobi (PCG) instantiation spills or touches scratch,
  - the PCG form of the default one-GPU shape 10821 (k_gemv_colsplit<8, 2, 4, MODE 2>) stays within 128 VGPRs, the budget that
    keeps it at 4 workgroups per CU (see the comment above k_gemv_colsplit),
  - every plain instantiation of the kernel families the feature touched keeps the VGPR / SGPR / LDS / scratch figures it had
    before the feature (pinned below from the tree the feature was built on)."""
import os
import re
import subprocess

import pytest

from test_kernel_resources import HIPCC, resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "conjugate-gradient_amd")

# (VGPRs, total SGPRs, LDS bytes per block, scratch bytes per lane) of the plain instantiations before the feature
PLAIN = {
    'cgx::k_close_iteration': (16, 21, 0, 0),
    'cgx::k_gemv_colsplit<1, 8, 4, 0, false, true>': (78, 32, 32, 0),
    'cgx::k_gemv_colsplit<1, 8, 4, 1, false, true>': (126, 52, 32, 0),
    'cgx::k_gemv_colsplit<16, 1, 4, 0, false, true>': (140, 64, 512, 0),
    'cgx::k_gemv_colsplit<16, 1, 4, 0, true, false>': (142, 56, 512, 0),
    'cgx::k_gemv_colsplit<16, 1, 4, 0, true, true>': (144, 62, 512, 0),
    'cgx::k_gemv_colsplit<16, 1, 4, 1, false, true>': (156, 74, 512, 0),
    'cgx::k_gemv_colsplit<16, 1, 4, 1, true, false>': (154, 72, 512, 0),
    'cgx::k_gemv_colsplit<16, 1, 4, 1, true, true>': (158, 74, 512, 0),
    'cgx::k_gemv_colsplit<2, 4, 4, 0, false, true>': (66, 34, 64, 0),
    'cgx::k_gemv_colsplit<2, 4, 4, 1, false, true>': (90, 52, 64, 0),
    'cgx::k_gemv_colsplit<2, 8, 4, 0, false, true>': (113, 34, 64, 0),
    'cgx::k_gemv_colsplit<2, 8, 4, 0, true, false>': (114, 30, 64, 0),
    'cgx::k_gemv_colsplit<2, 8, 4, 0, true, true>': (116, 34, 64, 0),
    'cgx::k_gemv_colsplit<2, 8, 4, 1, false, true>': (162, 46, 64, 0),
    'cgx::k_gemv_colsplit<2, 8, 4, 1, true, false>': (162, 44, 64, 0),
    'cgx::k_gemv_colsplit<2, 8, 4, 1, true, true>': (166, 46, 64, 0),
    'cgx::k_gemv_colsplit<4, 2, 4, 0, false, true>': (66, 38, 128, 0),
    'cgx::k_gemv_colsplit<4, 2, 4, 1, false, true>': (80, 56, 128, 0),
    'cgx::k_gemv_colsplit<4, 4, 4, 0, false, true>': (104, 38, 128, 0),
    'cgx::k_gemv_colsplit<4, 4, 4, 0, true, false>': (106, 34, 128, 0),
    'cgx::k_gemv_colsplit<4, 4, 4, 0, true, true>': (108, 38, 128, 0),
    'cgx::k_gemv_colsplit<4, 4, 4, 1, false, true>': (130, 50, 128, 0),
    'cgx::k_gemv_colsplit<4, 4, 4, 1, true, false>': (130, 48, 128, 0),
    'cgx::k_gemv_colsplit<4, 4, 4, 1, true, true>': (134, 50, 128, 0),
    'cgx::k_gemv_colsplit<8, 1, 4, 0, false, true>': (78, 46, 256, 0),
    'cgx::k_gemv_colsplit<8, 1, 4, 1, false, true>': (90, 64, 256, 0),
    'cgx::k_gemv_colsplit<8, 2, 4, 0, false, true>': (110, 48, 256, 0),
    'cgx::k_gemv_colsplit<8, 2, 4, 0, true, false>': (114, 44, 256, 0),
    'cgx::k_gemv_colsplit<8, 2, 4, 0, true, true>': (116, 46, 256, 0),
    'cgx::k_gemv_colsplit<8, 2, 4, 1, false, true>': (128, 58, 256, 0),
    'cgx::k_gemv_colsplit<8, 2, 4, 1, true, false>': (130, 56, 256, 0),
    'cgx::k_gemv_colsplit<8, 2, 4, 1, true, true>': (134, 58, 256, 0),
    'cgx::k_gemv_colsplit<8, 4, 4, 0, true, false>': (186, 44, 256, 0),
    'cgx::k_gemv_colsplit<8, 4, 4, 0, true, true>': (188, 46, 256, 0),
    'cgx::k_gemv_colsplit<8, 4, 4, 1, true, false>': (212, 56, 256, 0),
    'cgx::k_gemv_colsplit<8, 4, 4, 1, true, true>': (218, 58, 256, 0),
    'cgx::k_gemv_ldsp<1, 8, 4, 0>': (106, 36, 32800, 0),
    'cgx::k_gemv_ldsp<1, 8, 4, 1>': (125, 49, 32800, 0),
    'cgx::k_gemv_ldsp<16, 1, 4, 0>': (256, 34, 32800, 0),
    'cgx::k_gemv_ldsp<16, 1, 4, 1>': (256, 47, 32800, 0),
    'cgx::k_gemv_ldsp<2, 4, 4, 0>': (98, 36, 32800, 0),
    'cgx::k_gemv_ldsp<2, 4, 4, 1>': (118, 49, 32800, 0),
    'cgx::k_gemv_ldsp<2, 8, 4, 0>': (146, 37, 32800, 0),
    'cgx::k_gemv_ldsp<2, 8, 4, 1>': (166, 50, 32800, 0),
    'cgx::k_gemv_ldsp<4, 2, 4, 0>': (116, 36, 32800, 0),
    'cgx::k_gemv_ldsp<4, 2, 4, 1>': (136, 49, 32800, 0),
    'cgx::k_gemv_ldsp<4, 4, 4, 0>': (150, 36, 32800, 0),
    'cgx::k_gemv_ldsp<4, 4, 4, 1>': (170, 49, 32800, 0),
    'cgx::k_gemv_ldsp<8, 1, 4, 0>': (146, 34, 32800, 0),
    'cgx::k_gemv_ldsp<8, 1, 4, 1>': (166, 47, 32800, 0),
    'cgx::k_gemv_ldsp<8, 2, 4, 0>': (194, 36, 32800, 0),
    'cgx::k_gemv_ldsp<8, 2, 4, 1>': (212, 49, 32800, 0),
    'cgx::k_init_residual': (16, 44, 32, 0),
    'cgx::k_solve_begin_zero': (16, 52, 32, 0),
    'cgx::k_solve_end': (22, 20, 384, 0),
    'cgx::k_symv_tiles<256, false>': (120, 61, 20480, 0),
    'cgx::k_symv_tiles<256, true>': (123, 71, 20480, 0),
    'cgx::k_update_xr': (30, 42, 32, 0),
    'cgx::k_update_xr_p2p<false, false>': (58, 106, 288, 0),
    'cgx::k_update_xr_p2p<false, true>': (50, 100, 288, 0),
    'cgx::k_update_xr_p2p<true, false>': (62, 105, 288, 0),
    'cgx::k_update_xr_p2p<true, true>': (56, 99, 288, 0),
    'cgx::k_update_xr_strided': (22, 54, 32, 0),
}


def _all_resources():
    rows = {}
    for src in ("cgx_kernels.hip", "cgx_symv.hip", "cgx_p2p.hip"):
        for r in resources(src):
            rows[re.sub(r"\(.*", "", r["name"]).replace("void ", "")] = r
    return rows


@pytest.fixture(scope="module")
def kernel_rows():
    if not os.path.exists(HIPCC):
        pytest.skip("needs hipcc")
    return _all_resources()


def _is_pcg(name):
    if name.endswith("_pc") or "k_pcg_" in name:
        return True
    m = re.match(r"cgx::k_gemv_(colsplit|ldsp)<\d+, \d+, \d+, (\d+)", name)
    return bool(m) and m.group(2) == "2"   # MODE kFusedJacobi


def test_symbols_are_exported():
    lib = os.path.join(PKG, "libcgx.so")
    if not os.path.exists(lib):
        subprocess.check_call(["make", "-C", PKG, "-s", "all"])
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert {"cgx_set_preconditioner", "cgx_get_preconditioner"} <= syms


def test_header_constants_agree_with_python(pkg):
    text = open(os.path.join(ROOT, "include", "cgx.h")).read()
    consts = dict((k, int(v)) for k, v in re.findall(r"#define (CGX_PRECOND_\w+) (\d+)", text))
    assert consts == {"CGX_PRECOND_NONE": pkg.cgx.PRECOND_NONE, "CGX_PRECOND_JACOBI": pkg.cgx.PRECOND_JACOBI}
    assert re.search(r"cgx_status\s+cgx_set_preconditioner\(cgx_ctx \*ctx, int kind\);", text)
    assert re.search(r"cgx_status\s+cgx_get_preconditioner\(const cgx_ctx \*ctx, int \*kind\);", text)
    assert "cgx_set_preconditioner" in pkg.cgx.EXPORTS and "cgx_get_preconditioner" in pkg.cgx.EXPORTS


def test_python_rejects_an_unknown_kind_before_the_library(pkg):
    with pytest.raises(ValueError):
        pkg.CGSolver.set_preconditioner(object.__new__(pkg.CGSolver), "ilu")


def test_pcg_instantiations_never_spill(kernel_rows):
    pcg = {k: r for k, r in kernel_rows.items() if _is_pcg(k)}
    # every K1 family the library picks for dense storage has its Jacobi form, and so does every update kernel
    for want in ("cgx::k_gemv_colsplit<8, 2, 4, 2, false, true>", "cgx::k_gemv_colsplit<8, 2, 4, 2, true, false>",
                 "cgx::k_gemv_ldsp<4, 2, 4, 2>", "cgx::k_pcg_symv_tiles<256>", "cgx::k_update_xr_pc", "cgx::k_update_xr_strided_pc",
                 "cgx::k_init_residual_pc", "cgx::k_close_iteration_pc", "cgx::k_pcg_update_p2p<false>", "cgx::k_pcg_update_p2p<true>"):
        assert want in pcg, sorted(pcg)
    for k, r in pcg.items():
        assert int(r["VGPRs Spill"]) == 0 and int(r["SGPRs Spill"]) == 0 and int(r["ScratchSize [bytes/lane]"]) == 0, (k, r)


def test_pcg_form_of_the_default_shape_keeps_four_workgroups_per_cu(kernel_rows):
    r = kernel_rows["cgx::k_gemv_colsplit<8, 2, 4, 2, false, true>"]
    assert int(r["VGPRs"]) <= 128, r


# VGPRs of the Jacobi forms of K3 and of the residual set-up when each was a kernel text of its own; since they share their
# bodies with the plain and block forms (update_xr_tile, update_xr_strided, init_residual_rows) these are upper bounds
PC_VGPRS = {"cgx::k_update_xr_pc": 32, "cgx::k_update_xr_strided_pc": 30, "cgx::k_init_residual_pc": 22}


def test_jacobi_update_kernels_stay_within_their_vgprs(kernel_rows):
    for name, vgprs in PC_VGPRS.items():
        assert int(kernel_rows[name]["VGPRs"]) <= vgprs, (name, kernel_rows[name])


def test_plain_instantiations_keep_their_figures(kernel_rows):
    for name, (vgpr, sgpr, lds, scratch) in PLAIN.items():
        assert name in kernel_rows, name
        r = kernel_rows[name]
        got = (int(r["VGPRs"]), int(r["TotalSGPRs"]), int(r["LDS Size [bytes/block]"]), int(r["ScratchSize [bytes/lane]"]))
        assert got == (vgpr, sgpr, lds, scratch), (name, got)
