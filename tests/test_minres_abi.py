"""Build-time and host-only checks of MINRES (cgx_solve_minres): the argument check without a context, the header constant and its
Python mirror, the host reference that judges the GPU (tests/minres_reference.py) against np.linalg.solve and against its own
long-double run, the --minres argument errors of the CLI, and the register report of every kernel in csrc/cgx_minres.hip."""
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
