"""Build-time and host-only checks of the matrix-function entry points (cgx_tridiag_function, cgx_apply_function,
cgx_probe_funm_combine): the symbols and their prototypes, argument checks without a context, f(T) e_1 against
numpy.linalg.eigh, the restatement of tests/funm_reference.py against its references, the register report of csrc/cgx_funm.hip and
the argument checks of `cgsolver --apply`."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import funm_reference as fref
import lanczos_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
DP = C.POINTER(C.c_double)
ERR_BAD_ARG = 1
FNS = [(fref.FN_SQRT, 0.0), (fref.FN_INVSQRT, 0.0), (fref.FN_INV, 0.0), (fref.FN_LOG, 0.0), (fref.FN_EXP, 0.5)]


def _dp(a):
    return a.ctypes.data_as(DP)


def test_symbols_and_prototypes(pkg):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cgx.h")).read(), flags=re.S)
    flat = re.sub(r"\s+", " ", text)
    for proto in (
        "cgx_status cgx_tridiag_function(int m, const double *alpha, const double *beta, int fn, double param, double *coef, "
        "double *theta_minmax);",
        "cgx_status cgx_apply_function(cgx_ctx *ctx, int fn, double param, int nvec, int steps, const double *B, long ldb, double *X, "
        "long ldx, int *steps_done, double *change, double *coef);",
        "cgx_status cgx_probe_funm_combine(cgx_ctx *ctx, int nvec, int steps, const int *m, const double *Q, long ldq, const double *C, "
        "double *X, long ldx);",
    ):
        assert proto in flat, proto
    assert re.search(r"enum\s*\{\s*CGX_FN_SQRT\s*=\s*0\s*,\s*CGX_FN_INVSQRT\s*=\s*1\s*,\s*CGX_FN_INV\s*=\s*2\s*,\s*CGX_FN_LOG\s*=\s*3\s*,"
                     r"\s*CGX_FN_EXP\s*=\s*4\s*\}", text)
    cgx = pkg.cgx
    assert (cgx.FN_SQRT, cgx.FN_INVSQRT, cgx.FN_INV, cgx.FN_LOG, cgx.FN_EXP) == (0, 1, 2, 3, 4)
    assert (fref.FN_SQRT, fref.FN_INVSQRT, fref.FN_INV, fref.FN_LOG, fref.FN_EXP) == (0, 1, 2, 3, 4)
    out = subprocess.run(["nm", "-D", "--defined-only", cgx.LIB_PATH], capture_output=True, text=True).stdout
    for name in ("cgx_tridiag_function", "cgx_apply_function", "cgx_probe_funm_combine"):
        assert name in cgx.EXPORTS and re.search(r" T %s\b" % name, out), name
    assert hasattr(pkg.CGSolver, "apply_function") and hasattr(pkg.CGSolver, "_probe_funm_combine") and callable(cgx.tridiag_function)


def test_null_context_is_bad_arg(pkg):
    L = pkg.cgx.lib()
    b, x = np.ones(8), np.zeros(8)
    m = (C.c_int * 1)(1)
    assert L.cgx_apply_function(None, 0, 0.0, 1, 4, _dp(b), 8, _dp(x), 8, None, None, None) == ERR_BAD_ARG
    assert L.cgx_probe_funm_combine(None, 1, 1, m, _dp(b), 8, _dp(np.ones(1)), _dp(x), 8) == ERR_BAD_ARG
    assert np.all(x == 0.0)


def _check_function(pkg, alpha, beta, fn, param):
    """cgx_tridiag_function against Q f(Theta) Q^T e_1 from numpy.linalg.eigh of the dense T, in the 2-norm.  Both solvers are
    backward stable: each works with the exact eigen-decomposition of a matrix T + E_i, ||E_i|| <= 4 max(m, 4) eps ||T||_inf (the
    allowance of test_lanczos_abi._check_rule), so each returns f(T + E_i) e_1 up to the rounding of forming the product.  For a
    symmetric T, || f(T + E) - f(T) ||_F <= max |f'| ||E||_F over an interval holding both spectra, and ||E||_F <= sqrt(m) ||E||_2: the two
    results differ by at most 2 ||E|| sqrt(m) max |f'|.  Forming Q (f(theta) . q) and applying the rotations to g each keep the
    vector's norm to a few eps per entry's path: 4 eps ||c|| on top."""
    m = len(alpha)
    c, lo, hi = pkg.cgx.tridiag_function(alpha, beta, fn, param)
    T = ref.jacobi_matrix(alpha, beta, m)
    theta = np.linalg.eigvalsh(T)
    c_ref = fref.coefficients(alpha, beta, m, fn, param)
    norm = float(np.max(np.sum(np.abs(T), axis=1)))
    E = 4 * max(m, 4) * ref.EPS * norm
    assert abs(lo - theta[0]) <= 2 * E and abs(hi - theta[-1]) <= 2 * E, (m, lo - theta[0], hi - theta[-1])
    fmax = fref.derivative_bound(fn, param, theta[0] - E, theta[-1] + E)
    bound = 2 * E * np.sqrt(m) * fmax + 4 * ref.EPS * float(np.linalg.norm(c_ref))
    diff = float(np.linalg.norm(c - c_ref))
    print("m=%d fn=%s: ||c - c_ref|| = %.3e, bound %.3e (relative to ||c||: %.3e)" % (m, fref.NAMES[fn], diff, bound, diff / np.linalg.norm(c_ref)))
    assert diff <= bound, (m, fn, diff, bound)
    return c


@pytest.mark.parametrize("fn,param", FNS)
@pytest.mark.parametrize("m", [1, 2, 3, 50, 1024])
def test_tridiag_function_against_eigh(pkg, m, fn, param):
    rng = np.random.default_rng(100 + m)                      # the random T of test_lanczos_abi.py
    alpha = 2.0 + rng.random(m)
    beta = 0.25 + 0.5 * rng.random(max(m - 1, 0))
    _check_function(pkg, alpha, beta, fn, param)


@pytest.mark.parametrize("fn,param", FNS)
def test_tridiag_function_with_a_zero_beta(pkg, fn, param):
    """A beta of exactly 0 in the middle: f(T) e_1 is that of the leading block, every entry past the cut is exactly 0."""
    rng = np.random.default_rng(7)
    m, cut = 50, 20
    alpha = np.concatenate([2.0 + rng.random(cut), 10.0 + rng.random(m - cut)])
    beta = 0.25 + 0.5 * rng.random(m - 1)
    beta[cut - 1] = 0.0
    c = _check_function(pkg, alpha, beta, fn, param)
    assert np.all(c[cut:] == 0.0) and np.all(c[:cut] != 0.0)
    lead, _, _ = pkg.cgx.tridiag_function(alpha[:cut], beta[:cut - 1], fn, param)
    assert np.array_equal(c[:cut], lead)                      # the sweep of the leading block is the same sweep


def test_tridiag_function_leaves_beta_unread_for_m_1(pkg):
    L = pkg.cgx.lib()
    a, c, mm = np.array([4.0]), np.zeros(1), np.zeros(2)
    for fn, want in ((0, 2.0), (1, 0.5), (2, 0.25), (3, np.log(4.0)), (4, np.exp(-2.0))):
        assert L.cgx_tridiag_function(1, _dp(a), None, fn, 0.5, _dp(c), _dp(mm)) == 0
        assert c[0] == want and mm[0] == 4.0 and mm[1] == 4.0
    assert L.cgx_tridiag_function(1, _dp(a), None, 0, 0.0, _dp(c), None) == 0      # theta_minmax may be NULL


def test_tridiag_function_refusals(pkg):
    L = pkg.cgx.lib()
    a, b, c, mm = np.array([2.0, 3.0, 2.5]), np.array([0.5, 0.25]), np.zeros(3), np.zeros(2)
    call = L.cgx_tridiag_function
    assert call(3, _dp(a), _dp(b), 0, 0.0, _dp(c), _dp(mm)) == 0
    assert call(0, _dp(a), _dp(b), 0, 0.0, _dp(c), _dp(mm)) == ERR_BAD_ARG
    assert call(-1, _dp(a), _dp(b), 0, 0.0, _dp(c), _dp(mm)) == ERR_BAD_ARG
    assert call(3, None, _dp(b), 0, 0.0, _dp(c), _dp(mm)) == ERR_BAD_ARG
    assert call(3, _dp(a), None, 0, 0.0, _dp(c), _dp(mm)) == ERR_BAD_ARG
    assert call(3, _dp(a), _dp(b), 0, 0.0, None, _dp(mm)) == ERR_BAD_ARG
    for bad in (np.nan, np.inf, -np.inf):
        assert call(3, _dp(np.array([2.0, bad, 2.5])), _dp(b), 0, 0.0, _dp(c), _dp(mm)) == ERR_BAD_ARG
        assert call(3, _dp(a), _dp(np.array([0.5, bad])), 0, 0.0, _dp(c), _dp(mm)) == ERR_BAD_ARG
    for fn in (-1, 5, 100):
        assert call(3, _dp(a), _dp(b), fn, 0.0, _dp(c), _dp(mm)) == ERR_BAD_ARG
    for param in (-1.0, -1e-300, np.nan, np.inf):
        assert call(3, _dp(a), _dp(b), fref.FN_EXP, param, _dp(c), _dp(mm)) == ERR_BAD_ARG
        assert call(3, _dp(a), _dp(b), fref.FN_SQRT, param, _dp(c), _dp(mm)) == 0     # read for CGX_FN_EXP only
    assert call(3, _dp(a), _dp(b), fref.FN_EXP, 0.0, _dp(c), _dp(mm)) == 0 and np.allclose(c, [1.0, 0.0, 0.0], atol=1e-15)
    # the domain: T with the eigenvalues -1 and 3; theta_minmax is filled also when the call fails
    a2, b2 = np.array([1.0, 1.0]), np.array([2.0])
    for fn in (fref.FN_SQRT, fref.FN_INVSQRT, fref.FN_INV, fref.FN_LOG):
        mm[:] = 0.0
        assert call(2, _dp(a2), _dp(b2), fn, 0.0, _dp(c), _dp(mm)) == ERR_BAD_ARG
        assert abs(mm[0] + 1.0) <= 1e-14 and abs(mm[1] - 3.0) <= 1e-14
    assert call(2, _dp(a2), _dp(b2), fref.FN_EXP, 0.5, _dp(c), _dp(mm)) == 0
    # an eigenvalue of exactly 0: inside sqrt's domain, outside the others'
    zero = np.array([0.0])
    assert call(1, _dp(zero), None, fref.FN_SQRT, 0.0, _dp(c), _dp(mm)) == 0 and c[0] == 0.0
    for fn in (fref.FN_INVSQRT, fref.FN_INV, fref.FN_LOG):
        mm[:] = 1.0
        assert call(1, _dp(zero), None, fn, 0.0, _dp(c), _dp(mm)) == ERR_BAD_ARG and mm[0] == 0.0 and mm[1] == 0.0
    with pytest.raises(pkg.cgx.CgxError) as e:
        pkg.cgx.tridiag_function(a2, b2, fref.FN_LOG)
    assert e.value.status == ERR_BAD_ARG


def test_restatement_matches_the_references():
    """tests/funm_reference.py against itself on n = 120: the float64 restatement (coefficients through eigh) stays within the floor
    of the tolerance rule of Q f(Lambda) Q^T b once it has converged and of H f(D) H b in longdouble on an invariant subspace, and
    its change is || x_m - x_lag || / || x_m || while the Lanczos vectors are still orthogonal."""
    rng = np.random.default_rng(3)
    n = 120
    Qm, _ = np.linalg.qr(rng.standard_normal((n, n)))
    A = (Qm * np.linspace(1.0, 3.0, n)[None, :]) @ Qm.T
    A = 0.5 * (A + A.T)
    lam, Q = np.linalg.eigh(A)
    b = rng.standard_normal(n)
    run40, run10 = fref.lanczos_f64_basis(A, b, 40), fref.lanczos_f64_basis(A, b, 10)
    A4, H, d = ref.householder_matrix(n, [1.0, 3.0, 5.5, 9.0], 11)
    z = np.sign(rng.standard_normal(n))
    run4 = fref.lanczos_f64_basis(A4, z, 12)
    assert run40[2] == 40 and run4[2] == 4 and run4[3].shape == (4, n)
    for fn, param in FNS:
        x, c, chg = fref.combine(run40, fn, param)
        dev = fref.deviation(x, fref.eigh_reference(lam, Q, b, fn, param))
        print("%s: converged %.3e (change %.3e)" % (fref.NAMES[fn], dev, chg))
        assert dev <= ref.tolerance(0.0, n) and chg <= 1e-12
        x10, c10, chg10 = fref.combine(run10, fn, param)
        lag = fref.lag_of(10)
        x_lag = (np.sqrt(run10[4]) * fref.coefficients(run10[0], run10[1], lag, fn, param)) @ run10[3][:lag]
        exact = np.linalg.norm(x10 - x_lag) / np.linalg.norm(x10)
        # (x10 and x_lag are sums of 10 terms each, so their difference carries some 10 eps || x ||, and after 10 steps the
        # Lanczos vectors are orthogonal to ~ 1e-14: 1e-8 relative plus 64 * 10 eps absolute)
        assert lag == 9 and 1e-12 < chg10 < 1e-2 and abs(chg10 - exact) <= 1e-8 * exact + 640 * ref.EPS, (fn, chg10, exact)
        x4, _, _ = fref.combine(run4, fn, param)
        dev4 = fref.deviation(x4, fref.householder_reference(H, d, z, fn, param))
        print("%s: invariant subspace %.3e" % (fref.NAMES[fn], dev4))
        assert dev4 <= ref.tolerance(0.0, n)
    assert fref.change(np.array([3.0, 4.0]), np.zeros(0)) == 1.0 and fref.change(np.zeros(3), np.zeros(2)) == 0.0
    assert fref.change(np.array([3.0, 4.0]), np.array([3.0])) == 0.8
    assert [fref.lag_of(m) for m in (1, 2, 8, 16, 17, 120)] == [0, 1, 7, 14, 15, 105]


def _resources(src):
    """Per kernel: the compiler's resource report (-Rpass-analysis=kernel-resource-usage), names demangled."""
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"), "-c",
           os.path.join(ROOT, "conjugate-gradient_amd", "csrc", src), "-o", "/dev/null", "-Rpass-analysis=kernel-resource-usage"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    rows, cur = [], None
    for line in p.stderr.splitlines():
        m = re.search(r"remark:\s+([A-Za-z][A-Za-z \[\]/]*?):\s*(.*?) \[-Rpass", line)
        if not m:
            continue
        k, v = m.group(1).strip(), m.group(2).strip()
        if "Name" in k:
            cur = {"name": subprocess.run(["c++filt", v], capture_output=True, text=True).stdout.strip()}
            rows.append(cur)
        elif cur is not None:
            cur[k] = v
    return rows


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_funm_kernels_never_spill():
    rows = [r for r in _resources("cgx_funm.hip") if "cgx::" in r["name"]]
    names = sorted(re.search(r"(k_funm_\w+)", r["name"]).group(1) for r in rows)
    assert names == ["k_funm_combine"], [r["name"] for r in rows]
    for r in rows:
        print(r)
        assert int(r["VGPRs Spill"]) == 0 and int(r["ScratchSize [bytes/lane]"]) == 0, r
        assert int(r.get("SGPRs Spill", "0")) == 0, r


def test_cli_apply_argument_checks(pkg, tmp_path):
    exe = os.path.join(ROOT, "conjugate-gradient_amd", "cgsolver")
    out = str(tmp_path / "never_written.txt")
    takes, runs = "--apply takes", "--apply runs"
    for args, needle in ((["--apply", "cube"], takes), (["--apply", ""], takes), (["--apply", "sqrt,0"], takes), (["--apply", "sqrt,1025"], takes),
                         (["--apply", "sqrt,x"], takes), (["--apply", "sqrt,"], takes), (["--apply", "sqrt,10,0.5"], takes),
                         (["--apply", "exp,10,-1"], takes), (["--apply", "exp,10,x"], takes), (["--apply", "exp,10,inf"], takes),
                         (["--apply", "exp,10,1,2"], takes), (["--apply", "sqrt", "--jacobi"], runs), (["--apply", "sqrt", "--pivchol", "8"], runs),
                         (["--apply", "inv,8", "--shifts", "0,1"], runs), (["--apply", "log", "--logdet", "8"], runs)):
        r = subprocess.run([exe, "64", out] + args, capture_output=True, text=True)
        assert r.returncode == 1 and needle in r.stderr and "Usage" in r.stderr, (args, r.stderr[:300])
        assert not os.path.exists(out)
    assert "--apply NAME[,M[,T]]" in subprocess.run([exe], capture_output=True, text=True).stderr
