"""CPU checks of block Jacobi (include/cgx.h cgx_set_preconditioner_block): the two new entry points and
the probe are in the header, in cgx.py's EXPORTS and among the library's exported symbols; a null context is refused; Python
refuses a bad block size before the library is called; and a gfx950 cross-compile shows no spill and no scratch in any of the
new kernels (their figures are printed: DESIGN.md section 13 quotes them)."""
import ctypes as C
import os
import re
import subprocess

import pytest

from test_kernel_resources import HIPCC, resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "conjugate-gradient_amd")
NEW = ("cgx_set_preconditioner_block", "cgx_get_preconditioner_block", "cgx_probe_get_precond_blocks")
BLOCKS = (2, 4, 8, 16, 32, 64, 128, 256)
BAD_ARG = 1


def test_symbols_are_exported_declared_and_bound(pkg):
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.cgx.LIB_PATH], capture_output=True, text=True, check=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    text = open(os.path.join(ROOT, "include", "cgx.h")).read()
    for name in NEW:
        assert name in syms and name in pkg.cgx.EXPORTS, name
    assert re.search(r"cgx_status\s+cgx_set_preconditioner_block\(cgx_ctx \*ctx, int block\);", text)
    assert re.search(r"cgx_status\s+cgx_get_preconditioner_block\(const cgx_ctx \*ctx, int \*block\);", text)
    assert re.search(r"cgx_status\s+cgx_probe_get_precond_blocks\(cgx_ctx \*ctx, int local_shard, double \*W_out\);", text)
    # the block size is a parameter of the Jacobi kind, not a kind of its own
    assert sorted(re.findall(r"#define (CGX_PRECOND_\w+)", text)) == ["CGX_PRECOND_JACOBI", "CGX_PRECOND_NONE"]


def test_null_context_is_refused(pkg):
    L = pkg.cgx.lib()
    b = C.c_int(7)
    w = (C.c_double * 4)()
    assert L.cgx_set_preconditioner_block(None, 4) == BAD_ARG
    assert L.cgx_get_preconditioner_block(None, C.byref(b)) == BAD_ARG
    assert L.cgx_probe_get_precond_blocks(None, 0, w) == BAD_ARG


@pytest.mark.parametrize("block", [0, 3, 512, -1])
def test_python_rejects_a_bad_block_before_the_library(pkg, block):
    s = object.__new__(pkg.CGSolver)   # no handle: reaching the library would fail differently
    with pytest.raises(ValueError):
        pkg.CGSolver.set_preconditioner(s, "jacobi", block=block)
    with pytest.raises(ValueError):
        pkg.CGSolver.set_preconditioner(s, "jacobi", block=2.0)


def test_cli_names_the_switch(pkg):
    usage = subprocess.run([os.path.join(PKG, "cgsolver")], capture_output=True, text=True, timeout=60)
    assert "--jacobi-block" in usage.stderr
    assert "set_preconditioner_block" in open(os.path.join(PKG, "host", "cg.hh")).read()


@pytest.fixture(scope="module")
def new_kernels():
    if not os.path.exists(HIPCC):
        pytest.skip("needs hipcc")
    rows = {}
    for src in ("cgx_kernels.hip", "cgx_csr.hip"):
        for r in resources(src):
            name = re.sub(r"\(.*", "", r["name"].replace("(anonymous namespace)::", "")).replace("void ", "")
            if "_bj" in name:
                rows[name] = r
    return rows


def test_new_kernels_never_spill(new_kernels):
    want = ["cgx::k_bj_col_slice", "cgx::k_csr_bj_col_slice", "cgx::k_bj_invert<true>", "cgx::k_bj_invert<false>"]
    for b in BLOCKS:
        want += ["cgx::k_update_xr_bj<%d>" % b, "cgx::k_update_xr_strided_bj<%d>" % b, "cgx::k_init_residual_bj<%d>" % b]
    assert sorted(new_kernels) == sorted(want)
    for name in want:
        r = new_kernels[name]
        print("%-40s VGPRs %3d  SGPRs %3d  LDS %5d B" % (name, int(r["VGPRs"]), int(r["TotalSGPRs"]), int(r["LDS Size [bytes/block]"])))
        assert int(r["VGPRs Spill"]) == 0 and int(r["SGPRs Spill"]) == 0 and int(r["ScratchSize [bytes/lane]"]) == 0, (name, r)
    # the update kernels keep to the registers of eight waves per SIMD (64 VGPRs would be the plain kernel's class; 128 is
    # what 256 threads x 4 workgroups per CU allow): none of them needs more
    for b in BLOCKS:
        assert int(new_kernels["cgx::k_update_xr_bj<%d>" % b]["VGPRs"]) <= 128


# VGPRs per block size (BLOCKS order) when every block form was a kernel text of its own; since they share their bodies with
# the plain and Jacobi forms (update_xr_tile, update_xr_strided, init_residual_rows in cgx_kernels.hip) these are upper bounds
BJ_VGPRS = {
    "cgx::k_update_xr_bj": (34, 38, 52, 70, 70, 70, 70, 70),
    "cgx::k_update_xr_strided_bj": (36, 42, 56, 74, 68, 68, 68, 66),
    "cgx::k_init_residual_bj": (28, 34, 48, 68, 64, 64, 64, 62),
}


def test_block_forms_stay_within_their_vgprs(new_kernels):
    for kernel, bounds in BJ_VGPRS.items():
        for b, vgprs in zip(BLOCKS, bounds):
            r = new_kernels["%s<%d>" % (kernel, b)]
            assert int(r["VGPRs"]) <= vgprs, (kernel, b, r)
