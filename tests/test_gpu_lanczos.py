"""cgx_lanczos / cgx_trace_slq (csrc/cgx_lanczos.hip) on the MI355X.

- the coefficients against a longdouble Lanczos with full reorthogonalisation on the symmetric hash matrix;
- breakdown and freezing on A = H D H with 4 and 8 distinct eigenvalues, beside columns that run on;
- exact quadrature on a diagonal matrix, converged quadrature on the hash matrix, the log det of a kernel matrix;
- the library's probes, determinism, permutations; no interference with the single and multi paths; refusals; the fault walk.

The tolerance rule: wherever a device value is compared with a high-precision reference, the test computes d_cpu, the deviation of
the float64 numpy restatement of the same recurrence (tests/lanczos_reference.py) from that reference, and allows the device
16 max(d_cpu, n 2^-52) relative to max |alpha| or to the reference value (lanczos_reference.tolerance).

Past 16 row tiles and 256 K1 partials (n = 4100 .. 16400): tests/test_gpu_lanczos_tiles.py.
"""
import ctypes as C

import numpy as np
import pytest

import lanczos_reference as ref
import pivchol_reference

pytestmark = pytest.mark.gpu

SEED = 0x3D1F
ERR_BAD_ARG, ERR_HIP, ERR_UNSUPPORTED = 1, 3, 7   # cgx_status (include/cgx.h)
STEPS = 24
_CACHE = {}


def _diag(n):
    return 1.03 * 2.0 * np.sqrt(n / 3.0)   # the diagonal of tests/test_gpu_multi_rhs.py: the hash matrix is SPD


def _hash_solver(pkg, n, **kw):
    s = pkg.CGSolver(gemv_variant=kw.pop("gemv_variant", -1), **kw)
    s.generate_lap2d_matrix(n)
    s.probe_fill_matrix_hash(SEED, symmetric=True, diag=_diag(n))
    return s


def _dense_solver(pkg, A):
    s = pkg.CGSolver(gemv_variant=-1)
    s.set_matrix_dense(A)
    return s


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _hash_case(oracle, n):
    """Made once per n and left unchanged: the matrix, 16 start vectors, and per vector the longdouble reference and the float64
    restatement of STEPS steps."""
    if ("hash", n) not in _CACHE:
        A = oracle.hash_rows_numpy(n, np.arange(n), SEED, True, _diag(n))
        V0 = np.random.default_rng(1000 + n).standard_normal((16, n))
        Al = A.astype(np.longdouble)
        hi = [ref.lanczos_longdouble(Al, V0[j], STEPS) for j in range(16)]
        a_ref = np.array([h[0] for h in hi])
        b_ref = np.array([h[1] for h in hi])
        cpu = [ref.lanczos_f64(A, V0[j], STEPS) for j in range(16)]
        assert all(c[2] == STEPS for c in cpu)
        a_cpu = np.array([c[0] for c in cpu])
        b_cpu = np.array([c[1] for c in cpu])
        _CACHE[("hash", n)] = _frozen(A, V0, a_ref, b_ref, a_cpu, b_cpu)
    return _CACHE[("hash", n)]


# ---- 1. the coefficients ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nvec", [1, 3, 8, 16])
@pytest.mark.parametrize("n", [257, 1000])
def test_coefficients_against_longdouble(gpu_pkg, oracle, n, nvec):
    A, V0, a_ref, b_ref, a_cpu, b_cpu = _hash_case(oracle, n)
    with _hash_solver(gpu_pkg, n) as s:
        alpha, beta, done = s.lanczos(V0[:nvec], STEPS)
    _check_coefficients(n, nvec, STEPS, alpha, beta, done, a_ref, b_ref, a_cpu, b_cpu)


def _check_coefficients(n, nvec, steps, alpha, beta, done, a_ref, b_ref, a_cpu, b_cpu):
    """The device's (alpha, beta, done) of `steps` steps on nvec columns against the longdouble recurrence (a_ref, b_ref) under the
    rule, d_cpu from the float64 restatement (a_cpu, b_cpu).  Also run by tests/test_gpu_lanczos_tiles.py at n up to 16400."""
    assert list(done) == [steps] * nvec
    for j in range(nvec):
        scale = float(np.max(np.abs(a_ref[j])))
        d_cpu = float(max(np.max(np.abs(a_cpu[j] - a_ref[j])), np.max(np.abs(b_cpu[j] - b_ref[j])))) / scale
        d_dev = float(max(np.max(np.abs(alpha[j] - a_ref[j])), np.max(np.abs(beta[j] - b_ref[j])))) / scale
        print("coefficients n=%d nvec=%d column %d: d_cpu=%.3e d_dev=%.3e tol=%.3e" % (n, nvec, j, d_cpu, d_dev, ref.tolerance(d_cpu, n)))
        assert d_dev <= ref.tolerance(d_cpu, n), (n, nvec, j, d_cpu, d_dev)


# ---- 2. breakdown and freezing ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nd", [4, 8])
def test_breakdown_and_freezing(gpu_pkg, nd):
    _breakdown_and_freezing(gpu_pkg, nd, 1000)


def _breakdown_and_freezing(gpu_pkg, nd, n):
    """(tests/test_gpu_lanczos_tiles.py runs it at n = 4100.)"""
    steps = 12
    A, H, d = ref.householder_matrix(n, np.linspace(1.0, 9.0, nd), 40 + nd)
    rng = np.random.default_rng(nd)
    Z = rng.choice([-1.0, 1.0], (3, n))
    i1, i2 = 1, nd - 1                                        # eigenvectors H e_i with d_i != 1: log d_i is not 0
    V = np.array([Z[0], H[:, i1], Z[1], H[:, i2]])
    with _dense_solver(gpu_pkg, A) as s:
        alpha, beta, done = s.lanczos(V, steps)
        alpha2, beta2, done2 = s.lanczos(Z, steps)            # no frozen companions, the same kernel width (4)
        out = s.logdet(steps=steps, Z=V)
    assert list(done) == [nd, 1, nd, 1], done
    assert list(done2) == [nd, nd, nd], done2
    for col, i in ((1, i1), (3, i2)):
        a_cpu, _, m_cpu = ref.lanczos_f64(A, V[col], steps)
        assert m_cpu == 1
        tol = ref.tolerance(abs(a_cpu[0] - d[i]) / d[i], n)
        print("eigenvector column %d: alpha_0 - d_i = %.3e (float64 %.3e)" % (col, alpha[col, 0] - d[i], a_cpu[0] - d[i]))
        assert abs(alpha[col, 0] - d[i]) <= tol * d[i]
        assert np.all(alpha[col, 1:] == 0) and np.all(beta[col, 1:] == 0)
    # the running columns beside the frozen ones: the bits of a call without them
    assert np.array_equal(alpha[0], alpha2[0]) and np.array_equal(beta[0], beta2[0])
    assert np.array_equal(alpha[2], alpha2[1]) and np.array_equal(beta[2], beta2[1])
    for j in (0, 2):
        amax = np.max(np.abs(alpha[j]))
        assert beta[j, nd - 1] <= ref.BREAK * amax and np.all(beta[j, :nd - 1] >= 0.1 * amax), beta[j]
        assert np.all(alpha[j, nd:] == 0) and np.all(beta[j, nd:] == 0)
    # the quadrature of each column is z^T log(A) z = sum_i log(d_i) (H z)_i^2
    Hl, dl = H.astype(np.longdouble), d.astype(np.longdouble)
    for j in range(4):
        x = Hl @ V[j].astype(np.longdouble)
        exact = float(np.sum(np.log(dl) * x * x))
        a_cpu, b_cpu, m_cpu = ref.lanczos_f64(A, V[j], steps)
        q_cpu = ref.quadrature(a_cpu, b_cpu, m_cpu, float(V[j] @ V[j]), np.log)
        d_cpu = abs(q_cpu - exact) / abs(exact)
        d_dev = abs(out["per_probe"][j] - exact) / abs(exact)
        print("H D H nd=%d column %d: d_cpu=%.3e d_dev=%.3e" % (nd, j, d_cpu, d_dev))
        assert d_dev <= ref.tolerance(d_cpu, n), (j, d_cpu, d_dev)


# ---- 3. exact quadrature ----------------------------------------------------------------------------------------------------------
def test_exact_quadrature_on_a_diagonal_matrix(gpu_pkg):
    n, steps, probes, seed = 1000, 12, 12, 5
    d = np.linspace(1.5, 9.0, 8)[np.arange(n) % 8]
    A = np.diag(d)
    Z = ref.rademacher(seed, probes, n)
    with _dense_solver(gpu_pkg, A) as s:
        out = {"log": s.logdet(probes=probes, steps=steps, seed=seed), "inv": s.trace_inv(probes=probes, steps=steps, seed=seed)}
    for key, f in (("log", np.log), ("inv", lambda t: 1.0 / t)):
        exact = float(np.sum(f(d.astype(np.longdouble))))
        d_cpu = 0.0
        for j in range(probes):
            a, b, m = ref.lanczos_f64(A, Z[j], steps)
            assert m == 8
            d_cpu = max(d_cpu, abs(ref.quadrature(a, b, m, float(Z[j] @ Z[j]), f) - exact) / abs(exact))
        tol = ref.tolerance(d_cpu, n)
        d_dev = np.max(np.abs(out[key]["per_probe"] - exact)) / abs(exact)
        print("diagonal matrix, %s: d_cpu=%.3e d_dev=%.3e std_error/|exact|=%.3e" % (key, d_cpu, d_dev, out[key]["std_error"] / abs(exact)))
        assert d_dev <= tol, (key, d_cpu, d_dev)
        assert abs(out[key]["estimate"] - exact) <= tol * abs(exact)
        assert out[key]["std_error"] <= tol * abs(exact)
        assert out[key]["ritz_min"] == pytest.approx(1.5, rel=1e-12) and out[key]["ritz_max"] == pytest.approx(9.0, rel=1e-12)


# ---- 4. converged quadrature ------------------------------------------------------------------------------------------------------
def test_converged_quadrature_on_the_hash_matrix(gpu_pkg, oracle):
    n = 1000
    A = _hash_case(oracle, n)[0]
    Z = np.random.default_rng(44).choice([-1.0, 1.0], (8, n))
    lam, Q = np.linalg.eigh(A)
    C2 = (Z @ Q) ** 2
    with _hash_solver(gpu_pkg, n) as s:
        out = {"log": s.logdet(steps=STEPS, Z=Z), "inv": s.trace_inv(steps=STEPS, Z=Z)}
    for key, f in (("log", np.log), ("inv", lambda t: 1.0 / t)):
        for j in range(8):
            exact = float(C2[j] @ f(lam))
            a, b, m = ref.lanczos_f64(A, Z[j], STEPS)
            d_cpu = abs(ref.quadrature(a, b, m, float(Z[j] @ Z[j]), f) - exact) / abs(exact)
            d_dev = abs(out[key]["per_probe"][j] - exact) / abs(exact)
            print("hash matrix, %s, probe %d: d_cpu=%.3e d_dev=%.3e" % (key, j, d_cpu, d_dev))
            assert d_dev <= ref.tolerance(d_cpu, n), (key, j, d_cpu, d_dev)


# ---- 5. the workload --------------------------------------------------------------------------------------------------------------
def test_logdet_of_a_kernel_matrix(gpu_pkg):
    n = 1024
    A, _ = pivchol_reference.kernel_matrix(n, 0.2, 1e-2)
    Z = np.random.default_rng(20261020).choice([-1., 1.], (16, n))
    sign, exact = np.linalg.slogdet(A)
    lam = np.linalg.eigvalsh(A)
    assert sign == 1.0
    with _dense_solver(gpu_pkg, A) as s:
        out = s.logdet(steps=120, Z=Z)
    print("kernel matrix: estimate %.6f slogdet %.6f, %.2f standard errors; std_error %.3f %% of |slogdet|; ritz_min / lambda_min "
          "%.6f, ritz_max / lambda_max - 1 = %.2e" % (out["estimate"], exact, abs(out["estimate"] - exact) / out["std_error"],
                                                     100 * out["std_error"] / abs(exact), out["ritz_min"] / lam[0],
                                                     out["ritz_max"] / lam[-1] - 1))
    assert abs(out["estimate"] - exact) <= 4 * out["std_error"]
    assert out["std_error"] <= 0.01 * abs(exact)
    assert abs(out["ritz_max"] - lam[-1]) <= 1e-10 * lam[-1]
    assert lam[0] * (1 - 1e-8) <= out["ritz_min"] <= 1.05 * lam[0]


# ---- 6. library probes and determinism --------------------------------------------------------------------------------------------
def _same(o1, o2):
    return all(np.array_equal(o1[k], o2[k]) for k in ("estimate", "std_error", "per_probe", "ritz_min", "ritz_max"))


def test_library_probes_and_determinism(gpu_pkg):
    n, probes, steps, seed = 257, 11, 20, 77
    Z = ref.rademacher(seed, probes, n)
    assert set(np.unique(Z)) == {-1.0, 1.0} and abs(Z.mean()) < 0.05
    perm = np.array([5, 2, 7, 0, 1, 6, 3, 4, 10, 8, 9])      # within the batches of 8 and 3
    with _hash_solver(gpu_pkg, n) as s:
        lib = s.logdet(probes=probes, steps=steps, seed=seed)
        own = s.logdet(steps=steps, Z=Z)
        again = s.logdet(probes=probes, steps=steps, seed=seed)
        other = s.logdet(probes=probes, steps=steps, seed=seed + 1)
        shuffled = s.logdet(steps=steps, Z=Z[perm])
    assert _same(lib, own) and _same(lib, again)
    assert not np.array_equal(lib["per_probe"], other["per_probe"])
    assert np.array_equal(shuffled["per_probe"], own["per_probe"][perm])
    assert lib["std_error"] == np.std(lib["per_probe"], ddof=1) / np.sqrt(probes) or \
        abs(lib["std_error"] - np.std(lib["per_probe"], ddof=1) / np.sqrt(probes)) <= 1e-12 * lib["std_error"]
    assert abs(lib["estimate"] - np.mean(lib["per_probe"])) <= 1e-14 * abs(lib["estimate"])
    with _hash_solver(gpu_pkg, n) as s:
        one = s.logdet(probes=1, steps=steps, seed=seed)
    assert one["std_error"] == 0.0 and one["estimate"] == one["per_probe"][0]


# ---- 7. no interference -----------------------------------------------------------------------------------------------------------
def test_no_interference_with_the_solves(gpu_pkg):
    n = 2048
    B = np.random.default_rng(9).standard_normal((5, n))
    runs = []
    for with_logdet in (False, True):
        with gpu_pkg.CGSolver(gemv_variant=-1) as s:
            s.generate_lap2d_matrix(n)
            s.init_source_term(1.0 / n)
            s.set_max_iter(200)
            plan = s.gemv_plan()
            if with_logdet:
                out = s.logdet(probes=9, steps=30)
                assert np.isfinite(out["estimate"]) and out["ritz_min"] > 0
                assert s.gemv_plan() == plan
            x = np.zeros(n)
            r = s.solve(x)
            X, res = s.solve_multi(B)
            assert s.gemv_plan() == plan
            runs.append((x, r, X, res))
    (x1, r1, X1, res1), (x2, r2, X2, res2) = runs
    assert np.array_equal(x1, x2) and np.array_equal(X1, X2)
    for key in ("iterations", "converged", "residual_prev", "residual_last", "x_norm", "rel_residual"):
        assert r1[key] == r2[key], key
        assert [q[key] for q in res1] == [q[key] for q in res2], key


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------------
def _refused(cgx, status, call, needle=None):
    with pytest.raises(cgx.CgxError) as e:
        call()
    assert e.value.status == status, e.value
    if needle is not None:
        assert needle in str(e.value), e.value


def _still_solves(s, n):
    s.init_source_term(1.0 / n)
    s.set_max_iter(5)
    x = np.zeros(n)
    assert s.solve(x)["iterations"] >= 1 and np.all(np.isfinite(x))


def test_refusals(gpu_pkg):
    cgx = gpu_pkg.cgx
    L = cgx.lib()
    n = 1100
    V = np.ones((2, n))
    # CGX_ERR_UNSUPPORTED: loopback ranks, banded and CSR storage, a preconditioner that is set
    for kw in (dict(comm_mode=cgx.COMM_LOOPBACK, nranks=2), dict(matrix_format=cgx.MATRIX_BANDED), dict(matrix_format=cgx.MATRIX_CSR)):
        with gpu_pkg.CGSolver(gemv_variant=-1, **kw) as s:
            s.generate_lap2d_matrix(n)
            _refused(cgx, ERR_UNSUPPORTED, lambda: s.lanczos(V, 4))
            _refused(cgx, ERR_UNSUPPORTED, lambda: s.logdet(probes=2, steps=4))
            _still_solves(s, n)
    with gpu_pkg.CGSolver(gemv_variant=-1) as s:
        _refused(cgx, ERR_BAD_ARG, lambda: s._trace_slq(cgx.SLQ_LOG, 2, 4, 1, None))          # no matrix
        s.generate_lap2d_matrix(n)
        for kind in ("jacobi", "pivchol"):
            s.set_preconditioner(kind)
            _refused(cgx, ERR_UNSUPPORTED, lambda: s.lanczos(V, 4), "preconditioner")
            _refused(cgx, ERR_UNSUPPORTED, lambda: s.trace_inv(probes=2, steps=4), "preconditioner")
        s.set_preconditioner(None)
        ref_out = s.lanczos(V, 4)
        # CGX_ERR_BAD_ARG, the context usable after each
        bad_calls = [
            lambda: s.lanczos(np.ones((0, n)), 4),
            lambda: s.lanczos(np.ones((17, n)), 4),
            lambda: s.logdet(probes=0, steps=4),
            lambda: s.logdet(probes=cgx.MAX_PROBES + 1, steps=4),
            lambda: s.lanczos(V, 0),
            lambda: s.lanczos(V, n + 1),                      # steps > n (and n + 1 > CGX_MAX_LANCZOS_STEPS)
            lambda: s.lanczos(V, cgx.MAX_LANCZOS_STEPS + 1),  # <= n, above the maximum
            lambda: s.logdet(probes=2, steps=0),
            lambda: s.logdet(probes=2, steps=cgx.MAX_LANCZOS_STEPS + 1),
            lambda: s._trace_slq(2, 2, 4, 1, None),           # unknown fn
            lambda: s._trace_slq(-1, 2, 4, 1, None),
        ]
        for k, call in enumerate(bad_calls):
            _refused(cgx, ERR_BAD_ARG, call)
            out = s.lanczos(V, 4)
            assert all(np.array_equal(a, b) for a, b in zip(out, ref_out)), k
        a, b = np.zeros((2, 4)), np.zeros((2, 4))
        done = (C.c_int * 2)()
        est, err = C.c_double(), C.c_double()
        dp = cgx._dp
        assert L.cgx_lanczos(s._h, 2, 4, dp(V), n - 1, dp(a), dp(b), done) == ERR_BAD_ARG       # ldv < n
        assert L.cgx_trace_slq(s._h, 0, 2, 4, 1, dp(V), n - 1, C.byref(est), C.byref(err), None, None) == ERR_BAD_ARG
        assert L.cgx_lanczos(s._h, 2, 4, None, n, dp(a), dp(b), done) == ERR_BAD_ARG            # null pointers
        assert L.cgx_lanczos(s._h, 2, 4, dp(V), n, None, dp(b), done) == ERR_BAD_ARG
        assert L.cgx_lanczos(s._h, 2, 4, dp(V), n, dp(a), None, done) == ERR_BAD_ARG
        assert L.cgx_lanczos(s._h, 2, 4, dp(V), n, dp(a), dp(b), None) == ERR_BAD_ARG
        assert L.cgx_trace_slq(s._h, 0, 2, 4, 1, None, 0, None, C.byref(err), None, None) == ERR_BAD_ARG
        assert L.cgx_trace_slq(s._h, 0, 2, 4, 1, None, 0, C.byref(est), None, None, None) == ERR_BAD_ARG
        # a start vector of norm 0 or not finite: the column is named
        for fill in (0.0, np.nan, np.inf):
            W = np.ones((3, n))
            W[1] = fill
            _refused(cgx, ERR_BAD_ARG, lambda: s.lanczos(W, 4), "start vector 1")
            Wp = np.ones((10, n))
            Wp[9] = fill
            _refused(cgx, ERR_BAD_ARG, lambda: s.logdet(steps=4, Z=Wp), "start vector 9")
            out = s.lanczos(V, 4)
            assert all(np.array_equal(a, b) for a, b in zip(out, ref_out))
        _still_solves(s, n)
    # not positive definite: a diagonal matrix with one entry -1
    m = 256
    d = np.full(m, 2.0)
    d[17] = -1.0
    with _dense_solver(gpu_pkg, np.diag(d)) as s:
        _refused(cgx, ERR_BAD_ARG, lambda: s.logdet(probes=2, steps=6), "matrix is not positive definite")
        _refused(cgx, ERR_BAD_ARG, lambda: s.trace_inv(probes=2, steps=6), "matrix is not positive definite")
        assert "-1.0" in L.cgx_last_error(s._h).decode()
        alpha, beta, done = s.lanczos(np.ones((1, m)), 6)     # the recurrence itself takes any symmetric matrix
        assert list(done) == [2]
        s.set_matrix_dense(np.diag(np.abs(d)))                # (CG itself needs a positive definite matrix)
        assert s.logdet(probes=2, steps=6)["estimate"] == pytest.approx(255 * np.log(2.0), rel=1e-12)
        _still_solves(s, m)


# ---- 9. error paths ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["lanczos", "logdet"])
def test_fault_walk(gpu_pkg, entry):
    cgx = gpu_pkg.cgx
    n, steps = 600, 4
    V = np.random.default_rng(2).standard_normal((3, n))

    def run(s):
        if entry == "lanczos":
            return s.lanczos(V, steps)
        o = s.logdet(probes=10, steps=steps, seed=3)          # two batches
        return o["per_probe"], np.array([o["estimate"], o["std_error"], o["ritz_min"], o["ritz_max"]])

    with gpu_pkg.CGSolver(gemv_variant=-1) as s:
        s.generate_lap2d_matrix(n)
        want = run(s)
    with gpu_pkg.CGSolver(gemv_variant=-1) as s:               # a fresh context: the walk also steps over the side block's making
        s.generate_lap2d_matrix(n)
        calls = 0
        while True:
            s._set_fault_after(calls)
            try:
                got = run(s)
            except cgx.CgxError as e:
                assert e.status == ERR_HIP, (calls, e)
                calls += 1
                assert calls < 200
                continue
            s._set_fault_after(-1)
            break
        assert calls >= (2 * steps + 6) * (1 if entry == "lanczos" else 2), calls
        assert all(np.array_equal(a, b) for a, b in zip(got, want))
        assert all(np.array_equal(a, b) for a, b in zip(run(s), want))
        _still_solves(s, n)


# ---- the command line -------------------------------------------------------------------------------------------------------------
def test_cli_logdet_prints_the_library_call(gpu_pkg, tmp_path):
    import os
    import re
    import subprocess
    n, probes, steps = 1024, 8, 40
    exe = os.path.join(os.path.dirname(gpu_pkg.cgx.LIB_PATH), "cgsolver")
    out = tmp_path / "times.csv"
    r = subprocess.run([exe, str(n), str(out), "--logdet", "%d,%d" % (probes, steps)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if "[LOGDET]" in ln]
    assert len(lines) == 1, r.stdout
    m = re.search(r"probes = (\d+), steps = (\d+), log det A = (\S+), standard error = (\S+), Ritz values in \[(\S+), (\S+)\]", lines[0])
    assert m and (int(m.group(1)), int(m.group(2))) == (probes, steps), lines[0]
    assert out.read_text().startswith("%d,1," % n)
    with gpu_pkg.CGSolver(gemv_variant=-1) as s:
        s.generate_lap2d_matrix(n)
        want = s.logdet(probes=probes, steps=steps, seed=1)
    assert float(m.group(3)) == pytest.approx(want["estimate"], rel=1e-11)         # printed with 12 digits
    assert float(m.group(4)) == pytest.approx(want["std_error"], rel=1e-5)         # ... and 6
    assert float(m.group(5)) == pytest.approx(want["ritz_min"], rel=1e-5) and float(m.group(6)) == pytest.approx(want["ritz_max"], rel=1e-5)
