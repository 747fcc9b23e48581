"""Build-time and host-only checks of MINRES (cgx_solve_minres): the argument check without a context, the header constant and its
Python mirror, the host reference that judges the GPU (tests/minres_reference.py) against np.linalg.solve and against its own
long-double run and on every scenario of tests/test_gpu_minres_edges.py (the loop's ends on the 5-dimensional problem, shifts that
overflow, a source term that is zero or not finite, the hash matrix past 256 K1 partials, the 16 shifts of the long-vector run),
the --minres argument errors of the CLI, and the register report of every kernel in csrc/cgx_minres.hip."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import minres_reference as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


def test_null_context_is_bad_arg(pkg):
    L = pkg.cgx.lib()
    sig = np.zeros(2)
    X = np.zeros((2, 8))
    dp = C.POINTER(C.c_double)
    assert L.cgx_solve_minres(None, 2, sig.ctypes.data_as(dp), X.ctypes.data_as(dp), 8, None) == 1


def test_max_shifts_in_header_and_binding(pkg):
    text = open(os.path.join(ROOT, "include", "cgx.h")).read()
    m = re.search(r"#define\s+CGX_MAX_MINRES_SHIFTS\s+(\d+)", text)
    assert m and int(m.group(1)) == 16
    assert pkg.cgx.MAX_MINRES_SHIFTS == 16
    assert "cgx_solve_minres" in pkg.cgx.EXPORTS and hasattr(pkg.CGSolver, "solve_minres")


# ---- the reference, pinned before it judges the GPU ---------------------------------------------------------------------------------
def shifts_of(A):
    """The shift list of tests/test_gpu_minres.py: both signs, two interior ones at the midpoints of eigenvalues 3|4 and n-5|n-4,
    one beyond the spectrum."""
    ev = np.linalg.eigvalsh(A)
    n = len(ev)
    return [0.0, 1e-3, 1.0, 100.0, -0.5 * (ev[3] + ev[4]), -0.5 * (ev[n - 5] + ev[n - 4]), -(ev[-1] + 5.0), -1e4]


@pytest.mark.parametrize("n", [64, 257])
def test_reference_against_direct_solve(oracle, n):
    """Converged at tol 1e-10, every shift of the list: ||x - x*|| / ||x*|| <= 2 kappa rel_residual + 1e-13 kappa against
    np.linalg.solve (the standard bound, plus the host solve's own rounding), and a true relative residual of at most 5e-13: the
    recurrence's |phibar| < 1e-10 = 3e-14 ||b||, and the true residual drifts from it by rounding only."""
    A, b = oracle.generate_lap2d(n), oracle.init_source_term(n)
    S = shifts_of(A)
    for sigma, q in zip(S, mr.minres(A, b, S, n, 1e-10)):
        As = A + sigma * np.eye(n)
        xs = np.linalg.solve(As, b)
        true = np.linalg.norm(As @ q["x"] - b)
        kappa = np.linalg.cond(As)
        err = np.linalg.norm(q["x"] - xs) / np.linalg.norm(xs)
        print("n=%d sigma=%g: %d iterations, |phibar| %.3e, true %.3e, error %.2e, kappa %.2e" % (
            n, sigma, q["iterations"], q["residual_last"], true, err, kappa))
        assert q["converged"] == 1 and q["iterations"] < n and q["residual_last"] < 1e-10 <= q["residual_prev"], (sigma, q)
        assert true <= 5e-13 * np.linalg.norm(b), (sigma, true, q["residual_last"])
        assert err <= 2 * kappa * true / np.linalg.norm(b) + 1e-13 * kappa, (sigma, err)


@pytest.mark.parametrize("n", [64, 257, 1000])
def test_reference_float64_against_longdouble(oracle, n):
    """12 columns at tol 0: the float64 and the long-double run of the recurrence agree to 1e-13 relative in x -- 12 steps of a
    three-term recurrence whose every operation is accurate to a few eps = 2.2e-16 on well-separated scalars, a tenth of the
    1e-12 the GPU is held to -- also for a shift 2e-4 away from an eigenvalue; both count 12 iterations, unconverged."""
    A, b = oracle.generate_lap2d(n), oracle.init_source_term(n)
    S = shifts_of(A) + [-(np.linalg.eigvalsh(A)[2] + 2e-4)]
    lo, hi = mr.minres(A, b, S, 12, 0.0), mr.minres(A, b, S, 12, 0.0, np.longdouble)
    for sigma, q, p in zip(S, lo, hi):
        err = np.linalg.norm(q["x"] - p["x"]) / np.linalg.norm(p["x"])
        print("n=%d sigma=%g: float64 against long double %.2e" % (n, sigma, err))
        assert q["iterations"] == p["iterations"] == 12 and q["converged"] == p["converged"] == 0
        assert err <= 1e-13, (sigma, err)
        for key in ("residual_prev", "residual_last"):
            assert abs(q[key] - p[key]) <= 1e-12 * p[key], (sigma, key)
        assert q["residual_last"] <= q["residual_prev"] <= np.linalg.norm(b)   # monotone


def test_reference_csr_equals_dense():
    import test_gpu_csr as tc
    n = 300
    csr = tc.lap2d_csr(n)
    A = tc.csr_to_dense(*csr, n)
    b = np.cos(np.arange(n))
    for q, p in zip(mr.minres(csr, b, [0.0, -3.0], 12), mr.minres(A, b, [0.0, -3.0], 12)):
        assert np.linalg.norm(q["x"] - p["x"]) <= 1e-14 * np.linalg.norm(p["x"])


def test_reference_breakdown_and_singular_shifts():
    """A = diag(1, 2, 3, -4, -5 cycling), b = ones: the Krylov space has dimension 5, the recurrence breaks down in step 4.  Regular
    shifts end there with the exact solution; sigma = 4 and sigma = -2 make A + sigma I singular on that space."""
    n = 600
    d = np.array([1.0, 2.0, 3.0, -4.0, -5.0])[np.arange(n) % 5]
    res = mr.minres(np.diag(d), np.ones(n), [0.0, 0.5, 4.0, -2.0], n, 0.0)
    for sigma, q in zip([0.0, 0.5], res[:2]):
        assert (q["iterations"], q["converged"], q["residual_last"]) == (4, 1, 0.0), q
        assert np.abs(q["x"] - 1.0 / (d + sigma)).max() <= 1e-13
    for q in res[2:]:
        assert (q["iterations"], q["converged"]) == (4, 0) and np.isfinite(q["x"]).all(), q
    alone = mr.minres(np.diag(d), np.ones(n), [0.0, 0.5], n, 0.0)
    for q, p in zip(res[:2], alone):
        assert np.array_equal(q["x"], p["x"])
    zero = mr.minres(np.diag(d), np.zeros(n), [1.0], n, 1e-10)[0]
    assert (zero["iterations"], zero["converged"], zero["residual_last"]) == (0, 1, 0.0) and not zero["x"].any()


# ---- the scenarios of tests/test_gpu_minres_edges.py and the MINRES section of tests/test_gpu_row_pitch.py ---------------------------
DIAG5_SHIFTS = [0.0, 0.5, 4.0, -2.0]


def _diag5(n=600):
    return np.diag(np.array([1.0, 2.0, 3.0, -4.0, -5.0])[np.arange(n) % 5]), np.ones(n)


def _hash0(oracle, n):
    import test_gpu_minres as mn
    return oracle.hash_rows(n, 0, n, mn.SEED, True, 0.0), np.cos(np.arange(n, dtype=np.float64))


def test_reference_loop_ends_on_diag5():
    """The 5-dimensional problem cut at max_iter = 5 (the breakdown is found behind the last column), 4 (nothing breaks down: every
    shift runs out) and 0 (nothing runs: x = 0 and both residuals are ||b||; b = 0 is solved by x = 0 and counts as converged)."""
    A, b = _diag5()
    full = mr.minres(A, b, DIAG5_SHIFTS, 600, 0.0)
    five = mr.minres(A, b, DIAG5_SHIFTS, 5, 0.0)
    for q, p in zip(five, full):
        assert np.array_equal(q["x"], p["x"]) and all(q[k] == p[k] for k in ("iterations", "converged", "residual_prev", "residual_last"))
    assert [(q["iterations"], q["converged"]) for q in five] == [(4, 1), (4, 1), (4, 0), (4, 0)]
    assert five[0]["residual_last"] == five[1]["residual_last"] == 0.0
    four = mr.minres(A, b, DIAG5_SHIFTS, 4, 0.0)
    assert [(q["iterations"], q["converged"]) for q in four] == [(4, 0)] * 4
    for q, want in zip(four, (4.40, 3.55, 10.95, 10.95)):
        assert abs(q["residual_last"] - want) < 0.006 and q["residual_last"] <= q["residual_prev"], q
    nb = float(np.linalg.norm(b))
    for q in mr.minres(A, b, DIAG5_SHIFTS, 0, 0.0):
        assert (q["iterations"], q["converged"], q["residual_prev"], q["residual_last"]) == (0, 0, nb, nb) and not q["x"].any(), q
    for q in mr.minres(A, np.zeros(600), DIAG5_SHIFTS, 0, 0.0):
        assert (q["iterations"], q["converged"], q["residual_prev"], q["residual_last"]) == (0, 1, 0.0, 0.0) and not q["x"].any(), q


def test_reference_huge_shifts_and_infinite_source_term(oracle):
    """sigma = +-1e200 overflows gbar^2 in column 0: gamma is not finite and the shift freezes there, unconverged, with x = 0 and
    both residuals ||b||; the other shifts' bits do not change.  A b with an inf entry has no finite norm: nothing runs."""
    n = 513
    A, b = _hash0(oracle, n)
    res = mr.minres(A, b, [0.0, 1e200, -1e200, 1.0], 12, 0.0)
    nb = float(np.sqrt(b @ b))
    for q in res[1:3]:
        assert (q["iterations"], q["converged"], q["residual_prev"], q["residual_last"]) == (0, 0, nb, nb) and not q["x"].any(), q
    for q, p in zip((res[0], res[3]), mr.minres(A, b, [0.0, 1.0], 12, 0.0)):
        assert np.array_equal(q["x"], p["x"]) and (q["iterations"], q["converged"]) == (12, 0) == (p["iterations"], p["converged"])
        assert q["residual_last"] == p["residual_last"] < q["residual_prev"]
    binf = b.copy()
    binf[n // 2] = np.inf
    for q in mr.minres(A, binf, [0.0, -2.0], 12, 1e-10):
        assert (q["iterations"], q["converged"]) == (0, 0) and not q["x"].any(), q
        assert not np.isfinite(q["residual_prev"]) and not np.isfinite(q["residual_last"]), q


@pytest.mark.parametrize("n", [1028, 2052, 4100])
def test_reference_float64_against_longdouble_hash0(oracle, n):
    """The indefinite hash matrix past 256 K1 partials, 12 columns, minres_reference.tile_shifts (four of them interior)."""
    A, b = _hash0(oracle, n)
    S = mr.tile_shifts(n)
    lo, hi = mr.minres(A, b, S, 12, 0.0), mr.minres(A, b, S, 12, 0.0, np.longdouble)
    for sigma, q, p in zip(S, lo, hi):
        err = np.linalg.norm(q["x"] - p["x"]) / np.linalg.norm(p["x"])
        print("hash0 n=%d sigma=%g: float64 against long double %.2e" % (n, sigma, err))
        assert q["iterations"] == p["iterations"] == 12 and q["converged"] == p["converged"] == 0
        assert err <= 1e-13, (sigma, err)


def test_reference_long_shift_list():
    """minres_reference.LONG_SHIFTS on lap2d at 263501 rows: float64 against long double, the same freezes in both, and no freeze
    on the edge of the tolerance -- a device run whose |phibar| is off by 1e-9 relative freezes in the same columns."""
    import long_vector_reference as lv
    import test_gpu_csr as tc
    n, tol = lv.N_LONG, mr.LONG_TOL
    csr, b = tc.lap2d_csr(n), lv.normal_b(n)
    lo, hi = mr.minres(csr, b, mr.LONG_SHIFTS, 12, tol), mr.minres(csr, b, mr.LONG_SHIFTS, 12, tol, np.longdouble)
    for sigma, q, p in zip(mr.LONG_SHIFTS, lo, hi):
        err = np.linalg.norm(q["x"] - p["x"]) / np.linalg.norm(p["x"])
        print("long sigma=%g: (%d, %d), residual_prev %.3e, residual_last %.3e, float64 against long double %.2e" % (
            sigma, q["iterations"], q["converged"], q["residual_prev"], q["residual_last"], err))
        assert (q["iterations"], q["converged"]) == (p["iterations"], p["converged"]), (sigma, q, p)
        assert err <= 1e-13, (sigma, err)
        assert q["residual_last"] < 0.7 * tol or q["residual_last"] > 1.5 * tol, (sigma, q["residual_last"])
        assert q["converged"] == (1 if q["residual_last"] < tol else 0) and (not q["converged"] or q["residual_prev"] > 1.05 * tol), q
    got = {s: (q["iterations"], q["converged"]) for s, q in zip(mr.LONG_SHIFTS, lo)}
    assert [got[s] for s in (100.0, -20.0, -1e4, 30.0, 1e3)] == [(5, 1), (9, 1), (2, 1), (7, 1), (3, 1)], got
    assert all(got[s] == (12, 0) for s in (0.0, 1.0, -1.0, -3.7)), got
    assert sum(c for _, c in got.values()) == 8, got


# ---- the command line ---------------------------------------------------------------------------------------------------------------
def test_cli_minres_argument_errors(pkg, tmp_path):
    exe = os.path.join(ROOT, "conjugate-gradient_amd", "cgsolver")
    out = str(tmp_path / "never_written.txt")
    takes, two = "--minres takes", "two solvers"
    for args, needle in ((["--minres", "1,x"], takes), (["--minres", "1,,2"], takes), (["--minres", "-1,2e"], takes),
                         (["--minres", "0,-1", "--shifts", "0,1"], two), (["--shifts", "0,1", "--minres", "0,-1"], two),
                         (["--minres", "0", "--minres", "1"], two)):
        r = subprocess.run([exe, "64", out] + args, capture_output=True, text=True)
        assert r.returncode == 1 and needle in r.stderr and "Usage" in r.stderr, (args, r.stderr[:300])
        assert not os.path.exists(out)
    assert "--minres s0,s1,..." in subprocess.run([exe], capture_output=True, text=True).stderr


# ---- the register report ------------------------------------------------------------------------------------------------------------
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
def test_minres_kernels_never_spill():
    rows = [r for r in _resources("cgx_minres.hip") if "cgx::" in r["name"]]
    step = [r for r in rows if "k_minres_step" in r["name"]]
    assert len(step) == 5, [r["name"] for r in rows]     # widths 1, 2, 4, 8, 16
    assert len(rows) == 7, [r["name"] for r in rows]     # + init, close
    for r in rows:
        print(r["name"], r.get("VGPRs"), r.get("Occupancy [waves/SIMD]"))
        assert int(r["VGPRs Spill"]) == 0 and int(r["ScratchSize [bytes/lane]"]) == 0, r
