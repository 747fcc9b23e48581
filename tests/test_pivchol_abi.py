"""CPU checks of the pivoted-Cholesky preconditioner (include/cgx.h CGX_PRECOND_PIVCHOL): the new entry
points are declared, bound and exported; the kind is an enumerator with the value Python uses; a null context is refused; Python
refuses a bad rank or shift before the library is called; a gfx950 cross-compile of csrc/cgx_lowrank.hip shows no spill and no
scratch in any kernel (the figures are printed: DESIGN.md section 15 quotes them); and the numpy restatement of the set-up that
the GPU tests compare with (tests/pivchol_reference.py) holds its own bounds."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import pivchol_reference as ref
from test_kernel_resources import HIPCC, resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "conjugate-gradient_amd")
NEW = ("cgx_set_preconditioner_rank", "cgx_get_preconditioner_rank", "cgx_set_preconditioner_shift", "cgx_get_preconditioner_shift",
       "cgx_probe_get_precond_lowrank", "cgx_probe_precond_apply")
BAD_ARG = 1


def test_symbols_are_exported_declared_and_bound(pkg):
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.cgx.LIB_PATH], capture_output=True, text=True, check=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    text = open(os.path.join(ROOT, "include", "cgx.h")).read()
    for name in NEW:
        assert name in syms and name in pkg.cgx.EXPORTS, name
        assert re.search(r"cgx_status\s+%s\(" % name, text), name


def test_constants_match_the_header(pkg):
    text = open(os.path.join(ROOT, "include", "cgx.h")).read()
    m = re.search(r"enum\s*\{\s*CGX_PRECOND_PIVCHOL\s*=\s*(\d+)\s*\};", text)
    assert m and int(m.group(1)) == 2 == pkg.cgx.PRECOND_PIVCHOL
    assert not re.search(r"#define\s+CGX_PRECOND_PIVCHOL", text)
    m = re.search(r"#define\s+CGX_MAX_PRECOND_RANK\s+(\d+)", text)
    assert m and int(m.group(1)) == pkg.cgx.MAX_PRECOND_RANK == 256
    assert pkg.cgx._PRECOND_NAMES["pivchol"] == 2


def test_null_context_is_refused(pkg):
    L = pkg.cgx.lib()
    k = C.c_int(7)
    a, b = C.c_double(), C.c_double()
    v = (C.c_double * 4)()
    assert L.cgx_set_preconditioner_rank(None, 8) == BAD_ARG
    assert L.cgx_get_preconditioner_rank(None, C.byref(k)) == BAD_ARG
    assert L.cgx_set_preconditioner_shift(None, 0.5) == BAD_ARG
    assert L.cgx_get_preconditioner_shift(None, C.byref(a), C.byref(b)) == BAD_ARG
    assert L.cgx_probe_get_precond_lowrank(None, C.byref(k), v, C.byref(a)) == BAD_ARG
    assert L.cgx_probe_precond_apply(None, v, v) == BAD_ARG


@pytest.mark.parametrize("rank", [0, 257, 2.5, True, -3])
def test_python_rejects_a_bad_rank_before_the_library(pkg, rank):
    s = object.__new__(pkg.CGSolver)   # no handle: reaching the library would fail differently
    with pytest.raises(ValueError):
        pkg.CGSolver.set_preconditioner(s, "pivchol", rank=rank)


@pytest.mark.parametrize("shift", [-1.0, float("nan"), float("inf"), -0.5e-300, "1"])
def test_python_rejects_a_bad_shift_before_the_library(pkg, shift):
    s = object.__new__(pkg.CGSolver)
    with pytest.raises(ValueError):
        pkg.CGSolver.set_preconditioner(s, "pivchol", rank=8, shift=shift)


def test_python_keeps_the_block_validation_and_the_unknown_kind(pkg):
    s = object.__new__(pkg.CGSolver)
    with pytest.raises(ValueError):
        pkg.CGSolver.set_preconditioner(s, "pivchol", block=3)
    with pytest.raises(ValueError):
        pkg.CGSolver.set_preconditioner(s, "ichol")


def test_cli_and_mirror_name_the_switches(pkg):
    usage = subprocess.run([os.path.join(PKG, "cgsolver")], capture_output=True, text=True, timeout=60)
    assert "--pivchol K" in usage.stderr and "--pivchol-shift D" in usage.stderr
    hh = open(os.path.join(PKG, "host", "cg.hh")).read()
    assert "set_preconditioner_rank" in hh and "set_preconditioner_shift" in hh
    r = subprocess.run([os.path.join(PKG, "cgsolver"), "64", "/tmp/cgx_never_written.txt", "--pivchol", "300"], capture_output=True,
                       text=True, timeout=60)
    assert r.returncode == 1 and "--pivchol takes a rank" in r.stderr


@pytest.fixture(scope="module")
def lowrank_kernels():
    if not os.path.exists(HIPCC):
        pytest.skip("needs hipcc")
    rows = {}
    for r in resources("cgx_lowrank.hip"):
        rows[re.sub(r"\(.*", "", r["name"].replace("(anonymous namespace)::", "")).replace("void ", "")] = r
    return rows


def test_lowrank_kernels_never_spill(lowrank_kernels):
    want = ["cgx::k_lr_init", "cgx::k_lr_step", "cgx::k_lr_delta", "cgx::k_lr_gram", "cgx::k_lr_update<false>", "cgx::k_lr_update<true>",
            "cgx::k_lr_apply"]
    assert sorted(lowrank_kernels) == sorted(want)
    for name in want:
        r = lowrank_kernels[name]
        print("%-28s VGPRs %3d  SGPRs %3d  LDS %5d B" % (name, int(r["VGPRs"]), int(r["TotalSGPRs"]), int(r["LDS Size [bytes/block]"])))
        assert int(r["VGPRs Spill"]) == 0 and int(r["SGPRs Spill"]) == 0 and int(r["ScratchSize [bytes/lane]"]) == 0, (name, r)
    # the two kernels of the loop keep to the registers that 256 threads x 4 workgroups per CU allow, like block Jacobi's
    for name in ("cgx::k_lr_update<false>", "cgx::k_lr_apply"):
        assert int(lowrank_kernels[name]["VGPRs"]) <= 128, name


# ---- the numpy restatement of the set-up (the GPU tests compare the device's factor with the same checks) ----------------------
def test_restated_set_up_reproduces_the_pivot_rows():
    A, _ = ref.kernel_matrix(1024, 0.2, 1e-2)
    rank = 64
    piv, L, delta, d = ref.pivoted_cholesky(A, rank)
    assert len(set(piv.tolist())) == rank
    err = ref.pivot_row_error(A, piv, L)
    bar = 8 * rank * ref.EPS * np.abs(A).max()
    print("pivot rows: max |A - L L^T| = %.3e, bar %.3e" % (err, bar))
    assert err <= bar
    for t, p in enumerate(piv):
        assert np.all(L[piv[:t], t] == 0.0)              # rows chosen earlier: exactly 0
    ratio, mean_ld = ref.remaining_diagonal_checks(A, piv, L)
    print("smallest pivot / largest remaining diagonal = %.17g" % ratio)
    assert ratio >= 1.0 - 1e-9
    assert abs(ref.LD(delta) - mean_ld) <= 1e-8 * mean_ld
    assert ref.pivoted_cholesky(A, rank, shift=0.25)[2] == 0.25


def test_restated_woodbury_inverts_the_preconditioner():
    A, b = ref.kernel_matrix(1024, 0.2, 1e-2)
    _, L, delta, _ = ref.pivoted_cholesky(A, 64)
    z = ref.Woodbury(L, delta, ref.LD).apply(b)
    back = L.astype(ref.LD) @ (L.astype(ref.LD).T @ z) + ref.LD(delta) * z   # P z = b
    assert float(np.abs(back - b).max()) <= 1e-12 * float(np.abs(b).max())
