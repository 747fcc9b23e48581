"""cgx_apply_function / cgx_probe_funm_combine (csrc/cgx_funm.hip) on the MI355X.

- the combine kernel alone, exactly, on integer bases with non-finite values behind every column's last step;
- exact subspaces on A = H D H with 4 and 8 distinct eigenvalues, frozen columns beside running ones;
- converged (120 steps) and truncated (24 steps) results on the symmetric hash matrix against Q f(Lambda) Q^T b;
- consistency with cgx_lanczos_pc, cgx_tridiag_function, cgx_solve_multi and the multi-vector K1;
- determinism, permutations, no interference with the single and multi paths, refusals, the fault walk, the command line.

The tolerance rule is that of tests/test_gpu_lanczos.py: wherever a device result is compared with a reference, the test computes
d_cpu, the deviation of the float64 numpy restatement of the same computation (tests/funm_reference.py) from that reference, and
allows the device 16 max(d_cpu, n 2^-52), relative to the 2-norm of the reference (lanczos_reference.tolerance).  A truncated run
passes under the same rule because device and restatement share the truncation error.

Past 16 row tiles, 256 K1 partials and at 1024 steps of the combine (n = 4100): tests/test_gpu_lanczos_tiles.py.
"""
import os
import re
import subprocess

import numpy as np
import pytest

import funm_reference as fref
import lanczos_reference as ref

pytestmark = pytest.mark.gpu

SEED = 0x3D1F
ERR_BAD_ARG, ERR_HIP, ERR_UNSUPPORTED = 1, 3, 7   # cgx_status (include/cgx.h)
FNS = [(fref.FN_SQRT, 0.0), (fref.FN_INVSQRT, 0.0), (fref.FN_INV, 0.0), (fref.FN_LOG, 0.0), (fref.FN_EXP, 0.5)]
_CACHE = {}


def _diag(n):
    return 1.03 * 2.0 * np.sqrt(n / 3.0)   # the diagonal of tests/test_gpu_lanczos.py: the hash matrix is SPD


def _hash_solver(pkg, n, **kw):
    s = pkg.CGSolver(gemv_variant=kw.pop("gemv_variant", -1), **kw)
    s.generate_lap2d_matrix(n)
    s.probe_fill_matrix_hash(SEED, symmetric=True, diag=_diag(n))
    return s


def _dense_solver(pkg, A, **kw):
    s = pkg.CGSolver(gemv_variant=-1, **kw)
    s.set_matrix_dense(A)
    return s


def _hash_case(oracle, n):
    """Made once per n and left unchanged: the matrix, its eigen-decomposition and 16 vectors."""
    if ("hash", n) not in _CACHE:
        A = oracle.hash_rows_numpy(n, np.arange(n), SEED, True, _diag(n))
        lam, Q = np.linalg.eigh(A)
        B = np.random.default_rng(1000 + n).standard_normal((16, n))
        for a in (A, lam, Q, B):
            a.setflags(write=False)
        _CACHE[("hash", n)] = (A, lam, Q, B)
    return _CACHE[("hash", n)]


def _hash_runs(oracle, n, steps):
    """The restatement's kept runs of the 16 vectors, once per (n, steps): the functions share them."""
    if ("runs", n, steps) not in _CACHE:
        A, _, _, B = _hash_case(oracle, n)
        _CACHE[("runs", n, steps)] = [fref.lanczos_f64_basis(A, B[j], steps) for j in range(16)]
    return _CACHE[("runs", n, steps)]


# ---- 1. the combine kernel, exactly -----------------------------------------------------------------------------------------------
def _combine_case(s, rng, n, nvec, steps):
    Q = rng.integers(-8, 9, (steps, nvec, n)).astype(np.float64)
    Cf = rng.integers(-8, 9, (nvec, steps)).astype(np.float64)
    m = rng.integers(1, steps + 1, nvec).astype(np.int32)
    if nvec > 1:
        m[0], m[-1] = 1, steps
    want = np.array([Cf[j, :m[j]] @ Q[:m[j], j, :] for j in range(nvec)])   # integers below 2^53: every order is exact
    poison = [np.nan, np.inf, -np.inf]
    for j in range(nvec):
        for t in range(m[j], steps):
            Q[t, j, :] = poison[(t + j) % 3]
    got = s._probe_funm_combine(Q, Cf, m)
    assert np.array_equal(got, want), (n, nvec, steps, list(m), np.argwhere(got != want)[:4])


@pytest.mark.parametrize("n,lda_pad", [(1, -1), (255, -1), (257, -1), (1000, -1), (257, 0)])
def test_combine_is_exact(gpu_pkg, n, lda_pad):
    rng = np.random.default_rng(10 * n + lda_pad + 1)
    with _dense_solver(gpu_pkg, 2.0 * np.eye(n), lda_pad=lda_pad) as s:
        for steps in (1, 2, 37):                              # ascending: the side block is made again when a call needs more
            for nvec in (1, 3, 8, 16):
                _combine_case(s, rng, n, nvec, steps)
        _combine_case(s, rng, n, 2, 1)                        # ... and a smaller call reuses the larger block


# ---- 2. exact subspaces -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nd", [4, 8])
def test_exact_subspaces(gpu_pkg, nd):
    n, steps = 1000, 12
    A, H, d = ref.householder_matrix(n, np.linspace(1.0, 9.0, nd), 40 + nd)
    rng = np.random.default_rng(nd)
    Z = rng.choice([-1.0, 1.0], (3, n))
    i1, i2 = 1, nd - 1
    V = np.array([Z[0], H[:, i1], Z[1], H[:, i2]])
    with _dense_solver(gpu_pkg, A) as s:
        for fn, param in FNS:
            X, info = s.apply_function(V, fn, steps, param)
            X2, info2 = s.apply_function(Z, fn, steps, param)   # no frozen companions, the same kernel width (4)
            assert list(info["steps_done"]) == [nd, 1, nd, 1], info["steps_done"]
            assert list(info2["steps_done"]) == [nd, nd, nd]
            # the running columns beside the frozen ones: the bits of a call without them
            assert np.array_equal(X[0], X2[0]) and np.array_equal(X[2], X2[1])
            assert np.array_equal(info["coef"][0], info2["coef"][0]) and np.array_equal(info["coef"][2], info2["coef"][1])
            assert info["change"][0] == info2["change"][0] and info["change"][2] == info2["change"][1]
            assert np.all(info["coef"][:, nd:] == 0.0) and np.all(info["coef"][[1, 3], 1:] == 0.0)
            assert info["change"][1] == 1.0 and info["change"][3] == 1.0       # one step: lag = 0
            f = fref.scalar_function(fn, param)
            for j in range(4):
                x_ref = fref.householder_reference(H, d, V[j], fn, param)
                x_cpu, _, _ = fref.apply_f64(A, V[j], steps, fn, param)
                d_cpu, d_dev = fref.deviation(x_cpu, x_ref), fref.deviation(X[j], x_ref)
                tol = ref.tolerance(d_cpu, n)
                print("H D H nd=%d %s column %d: d_cpu=%.3e d_dev=%.3e tol=%.3e" % (nd, fref.NAMES[fn], j, d_cpu, d_dev, tol))
                assert d_dev <= tol, (nd, fn, j, d_cpu, d_dev)
            for col, i in ((1, i1), (3, i2)):                 # an eigenvector: f(d_i) times the vector
                x_eig = f(np.array([d[i]], dtype=np.longdouble))[0] * V[col].astype(np.longdouble)
                x_cpu, _, _ = fref.apply_f64(A, V[col], steps, fn, param)
                d_cpu, d_dev = fref.deviation(x_cpu, x_eig), fref.deviation(X[col], x_eig)
                print("H D H nd=%d %s eigenvector column %d: d_cpu=%.3e d_dev=%.3e" % (nd, fref.NAMES[fn], col, d_cpu, d_dev))
                assert d_dev <= ref.tolerance(d_cpu, n), (nd, fn, col, d_cpu, d_dev)


# ---- 3. converged and truncated ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("steps", [120, 24])
@pytest.mark.parametrize("nvec", [1, 3, 8, 16])
@pytest.mark.parametrize("n", [257, 1000])
def test_hash_matrix_against_eigh(gpu_pkg, oracle, n, nvec, steps):
    _hash_matrix_against_eigh(gpu_pkg, oracle, n, nvec, steps)


def _hash_matrix_against_eigh(gpu_pkg, oracle, n, nvec, steps):
    """(tests/test_gpu_lanczos_tiles.py runs it at n = 4100, with its own eigen-decomposition placed in _CACHE.)"""
    A, lam, Q, B = _hash_case(oracle, n)
    runs = _hash_runs(oracle, n, steps)
    with _hash_solver(gpu_pkg, n) as s:
        out = {fn: s.apply_function(B[:nvec], fn, steps, param) for fn, param in FNS}
    for fn, param in FNS:
        X, info = out[fn]
        assert list(info["steps_done"]) == [steps] * nvec
        worst = (0.0, 0.0, 0.0)
        for j in range(nvec):
            x_ref = fref.eigh_reference(lam, Q, B[j], fn, param)
            x_cpu, _, chg_cpu = fref.combine(runs[j], fn, param)
            d_cpu, d_dev = fref.deviation(x_cpu, x_ref), fref.deviation(X[j], x_ref)
            tol = ref.tolerance(d_cpu, n)
            worst = max(worst, (d_dev / tol, d_cpu, d_dev))
            print("hash n=%d nvec=%d steps=%d %s column %d: d_cpu=%.3e d_dev=%.3e tol=%.3e change=%.3e (float64 %.3e)"
                  % (n, nvec, steps, fref.NAMES[fn], j, d_cpu, d_dev, tol, info["change"][j], chg_cpu))
            assert d_dev <= tol, (n, nvec, steps, fn, j, d_cpu, d_dev)
        print("hash n=%d nvec=%d steps=%d %s: worst d_dev / tol = %.3f (d_cpu %.3e, d_dev %.3e)" % ((n, nvec, steps, fref.NAMES[fn]) + worst))


# ---- 4. consistency with the existing entry points --------------------------------------------------------------------------------
@pytest.mark.parametrize("nvec", [1, 3, 8, 16])
def test_coefficients_and_change_are_the_host_functions(gpu_pkg, oracle, nvec):
    n, steps = 257, 40
    cgx = gpu_pkg.cgx
    _, _, _, B = _hash_case(oracle, n)
    with _hash_solver(gpu_pkg, n) as s:
        alpha, beta, done, eta2 = s.lanczos_pc(B[:nvec], steps)          # no preconditioner set: cgx_lanczos, with ||B_j||^2
        out = {fn: s.apply_function(B[:nvec], fn, steps, param)[1] for fn, param in FNS}
    for fn, param in FNS:
        info = out[fn]
        assert np.array_equal(info["steps_done"], done)
        for j in range(nvec):
            m = int(done[j])
            scale = np.sqrt(eta2[j])
            c = scale * cgx.tridiag_function(alpha[j, :m], beta[j, :m], fn, param)[0]
            assert np.array_equal(info["coef"][j, :m], c) and np.all(info["coef"][j, m:] == 0.0), (fn, j)
            lag = fref.lag_of(m)
            c_lag = scale * cgx.tridiag_function(alpha[j, :lag], beta[j, :lag], fn, param)[0]
            assert info["change"][j] == fref.change(c, c_lag), (fn, j, info["change"][j], fref.change(c, c_lag))


def test_inverse_against_solve_multi(gpu_pkg, oracle):
    n, nvec, steps = 1000, 8, 120
    A, _, _, B = _hash_case(oracle, n)
    runs = _hash_runs(oracle, n, steps)
    with _hash_solver(gpu_pkg, n) as s:
        s.tolerance(1e-13)
        s.set_max_iter(400)
        Xcg, res = s.solve_multi(B[:nvec])
        X, _ = s.apply_function(B[:nvec], fref.FN_INV, steps)
    assert all(r["converged"] for r in res)
    for j in range(nvec):
        x_cpu, _, _ = fref.combine(runs[j], fref.FN_INV)
        d_cpu, d_dev = fref.deviation(x_cpu, Xcg[j]), fref.deviation(X[j], Xcg[j])
        print("INV against solve_multi, column %d: d_cpu=%.3e d_dev=%.3e tol=%.3e" % (j, d_cpu, d_dev, ref.tolerance(d_cpu, n)))
        assert d_dev <= ref.tolerance(d_cpu, n), (j, d_cpu, d_dev)


def test_square_root_twice_is_the_matrix(gpu_pkg, oracle):
    n, nvec, steps = 1000, 8, 120
    A, _, _, B = _hash_case(oracle, n)
    runs = _hash_runs(oracle, n, steps)
    with _hash_solver(gpu_pkg, n) as s:
        Y, pAp = s.probe_gemv_multi(B[:nvec])
        X1, _ = s.apply_function(B[:nvec], fref.FN_SQRT, steps)
        X2, _ = s.apply_function(X1, fref.FN_SQRT, steps)
    for j in range(nvec):
        h_cpu, _, _ = fref.combine(runs[j], fref.FN_SQRT)
        x_cpu, _, _ = fref.apply_f64(A, h_cpu, steps, fref.FN_SQRT)
        d_cpu, d_dev = fref.deviation(x_cpu, Y[j]), fref.deviation(X2[j], Y[j])
        print("sqrt twice against A b, column %d: d_cpu=%.3e d_dev=%.3e tol=%.3e" % (j, d_cpu, d_dev, ref.tolerance(d_cpu, n)))
        assert d_dev <= ref.tolerance(d_cpu, n), (j, d_cpu, d_dev)
        q_cpu, q_dev = abs(float(h_cpu @ h_cpu) - pAp[j]) / pAp[j], abs(float(X1[j] @ X1[j]) - pAp[j]) / pAp[j]
        print("||A^1/2 b||^2 against b.Ab, column %d: d_cpu=%.3e d_dev=%.3e" % (j, q_cpu, q_dev))
        assert q_dev <= ref.tolerance(q_cpu, n), (j, q_cpu, q_dev)


# ---- 5. determinism ---------------------------------------------------------------------------------------------------------------
def _same(o1, o2):
    return np.array_equal(o1[0], o2[0]) and all(np.array_equal(o1[1][k], o2[1][k]) for k in ("steps_done", "change", "coef"))


def test_determinism_and_permutations(gpu_pkg, oracle):
    n, steps = 257, 30
    _, _, _, B = _hash_case(oracle, n)
    perm = np.array([5, 2, 7, 0, 1, 6, 3, 4])
    bad = np.array(B[:8])
    bad[3, 100] = np.inf
    with _hash_solver(gpu_pkg, n) as s:
        first = s.apply_function(B[:8], fref.FN_INVSQRT, steps)
        again = s.apply_function(B[:8], fref.FN_INVSQRT, steps)
        shuffled = s.apply_function(B[:8][perm], fref.FN_INVSQRT, steps)
    assert _same(first, again)
    assert np.array_equal(shuffled[0], first[0][perm])
    assert np.array_equal(shuffled[1]["coef"], first[1]["coef"][perm]) and np.array_equal(shuffled[1]["change"], first[1]["change"][perm])
    with _hash_solver(gpu_pkg, n) as s:
        with pytest.raises(gpu_pkg.cgx.CgxError) as e:        # the refused call leaves inf / nan in the kept basis
            s.apply_function(bad, fref.FN_INVSQRT, steps)
        assert e.value.status == ERR_BAD_ARG and "start vector 3" in str(e.value)
        after = s.apply_function(B[:8], fref.FN_INVSQRT, steps)
    assert _same(first, after)                                # 'first' came from a fresh context


# ---- 6. no interference -----------------------------------------------------------------------------------------------------------
def test_no_interference_with_the_solves(gpu_pkg):
    n = 2048
    B = np.random.default_rng(9).standard_normal((5, n))
    runs = []
    for with_apply in (False, True):
        with gpu_pkg.CGSolver(gemv_variant=-1) as s:
            s.generate_lap2d_matrix(n)
            s.init_source_term(1.0 / n)
            s.set_max_iter(200)
            plan = s.gemv_plan()
            if with_apply:
                X, info = s.apply_function(B, fref.FN_SQRT, 30)
                assert np.all(np.isfinite(X)) and list(info["steps_done"]) == [30] * 5
                assert s.gemv_plan() == plan
            x = np.zeros(n)
            r = s.solve(x)
            Xm, res = s.solve_multi(B)
            lz = s.lanczos(B, 20)
            assert s.gemv_plan() == plan
            runs.append((x, r, Xm, res, lz))
    (x1, r1, X1, res1, lz1), (x2, r2, X2, res2, lz2) = runs
    assert np.array_equal(x1, x2) and np.array_equal(X1, X2)
    assert all(np.array_equal(a, b) for a, b in zip(lz1, lz2))
    for key in ("iterations", "converged", "residual_prev", "residual_last", "x_norm", "rel_residual"):
        assert r1[key] == r2[key], key
        assert [q[key] for q in res1] == [q[key] for q in res2], key


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------
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
    V[1, ::2] = -1.0
    # CGX_ERR_UNSUPPORTED: loopback ranks, banded and CSR storage, a preconditioner that is set
    for kw in (dict(comm_mode=cgx.COMM_LOOPBACK, nranks=2), dict(matrix_format=cgx.MATRIX_BANDED), dict(matrix_format=cgx.MATRIX_CSR)):
        with gpu_pkg.CGSolver(gemv_variant=-1, **kw) as s:
            s.generate_lap2d_matrix(n)
            _refused(cgx, ERR_UNSUPPORTED, lambda: s.apply_function(V, cgx.FN_SQRT, 4))
            _still_solves(s, n)
    with gpu_pkg.CGSolver(gemv_variant=-1) as s:
        X0 = np.zeros_like(V)
        assert L.cgx_apply_function(s._h, 0, 0.0, 2, 4, cgx._dp(V), n, cgx._dp(X0), n, None, None, None) == ERR_BAD_ARG   # no matrix
        s.generate_lap2d_matrix(n)
        for kind in ("jacobi", "pivchol"):
            s.set_preconditioner(kind)
            _refused(cgx, ERR_UNSUPPORTED, lambda: s.apply_function(V, cgx.FN_SQRT, 4), "preconditioner")
        s.set_preconditioner(None)
        ref_out = s.apply_function(V, cgx.FN_SQRT, 4)

        def good(k):
            assert _same(s.apply_function(V, cgx.FN_SQRT, 4), ref_out), k

        # CGX_ERR_BAD_ARG, a successful call on the same context after each
        bad_calls = [
            lambda: s.apply_function(np.ones((0, n)), cgx.FN_SQRT, 4),
            lambda: s.apply_function(np.ones((17, n)), cgx.FN_SQRT, 4),
            lambda: s.apply_function(V, cgx.FN_SQRT, 0),
            lambda: s.apply_function(V, cgx.FN_SQRT, n + 1),                      # steps > n (and above the maximum)
            lambda: s.apply_function(V, cgx.FN_SQRT, cgx.MAX_LANCZOS_STEPS + 1),  # <= n, above the maximum
            lambda: s.apply_function(V, -1, 4),
            lambda: s.apply_function(V, 5, 4),
            lambda: s.apply_function(V, cgx.FN_EXP, 4, -1.0),
            lambda: s.apply_function(V, cgx.FN_EXP, 4, np.nan),
            lambda: s.apply_function(V, cgx.FN_EXP, 4, np.inf),
        ]
        for k, call in enumerate(bad_calls):
            _refused(cgx, ERR_BAD_ARG, call)
            good(k)
        assert np.all(np.isfinite(s.apply_function(V, cgx.FN_SQRT, 4, np.nan)[0]))     # param is read for FN_EXP only
        X = np.zeros_like(V)
        dp = cgx._dp
        call = L.cgx_apply_function
        assert call(s._h, 0, 0.0, 2, 4, dp(V), n - 1, dp(X), n, None, None, None) == ERR_BAD_ARG    # ldb < n
        assert call(s._h, 0, 0.0, 2, 4, dp(V), n, dp(X), n - 1, None, None, None) == ERR_BAD_ARG    # ldx < n
        assert call(s._h, 0, 0.0, 2, 4, None, n, dp(X), n, None, None, None) == ERR_BAD_ARG         # null pointers
        assert call(s._h, 0, 0.0, 2, 4, dp(V), n, None, n, None, None, None) == ERR_BAD_ARG
        assert np.all(X == 0.0)
        assert call(s._h, 0, 0.0, 2, 4, dp(V), n, dp(X), n, None, None, None) == 0                  # the three outputs may be NULL
        assert np.array_equal(X, ref_out[0])
        good("raw")
        # a start vector of norm 0 or not finite: the column is named, X is not written
        for fill in (0.0, np.nan, np.inf):
            W = np.ones((3, n))
            W[1] = fill
            X3 = np.full((3, n), 7.0)
            st = call(s._h, 0, 0.0, 3, 4, dp(W), n, dp(X3), n, None, None, None)
            assert st == ERR_BAD_ARG and "start vector 1" in L.cgx_last_error(s._h).decode() and np.all(X3 == 7.0)
            good(fill)
        _still_solves(s, n)
    # not positive definite: H D H with one negative d; exp takes any symmetric matrix
    m = 256
    dvals = np.linspace(1.0, 4.0, 8)
    dvals[3] = -1.0
    A, H, d = ref.householder_matrix(m, dvals, 5)
    Z = np.random.default_rng(6).choice([-1.0, 1.0], (2, m))
    with _dense_solver(gpu_pkg, A) as s:
        for fn in (cgx.FN_SQRT, cgx.FN_INVSQRT, cgx.FN_INV, cgx.FN_LOG):
            _refused(cgx, ERR_BAD_ARG, lambda: s.apply_function(Z, fn, 12), "matrix is not positive definite")
            msg = L.cgx_last_error(s._h).decode()
            assert "-1.0" in msg and "column 0" in msg, msg
        X, info = s.apply_function(Z, cgx.FN_EXP, 12, 0.25)
        assert list(info["steps_done"]) == [8, 8]
        for j in range(2):
            x_ref = fref.householder_reference(H, d, Z[j], cgx.FN_EXP, 0.25)
            x_cpu, _, _ = fref.apply_f64(A, Z[j], 12, cgx.FN_EXP, 0.25)
            d_cpu, d_dev = fref.deviation(x_cpu, x_ref), fref.deviation(X[j], x_ref)
            print("exp on an indefinite H D H, column %d: d_cpu=%.3e d_dev=%.3e" % (j, d_cpu, d_dev))
            assert d_dev <= ref.tolerance(d_cpu, m)
        s.set_matrix_dense(np.diag(np.abs(d)))                # (CG itself needs a positive definite matrix)
        _still_solves(s, m)


# ---- 8. error paths ---------------------------------------------------------------------------------------------------------------
def test_fault_walk(gpu_pkg):
    cgx = gpu_pkg.cgx
    n, steps = 600, 4
    V = np.random.default_rng(2).standard_normal((3, n))

    def run(s):
        return s.apply_function(V, cgx.FN_LOG, steps)

    with gpu_pkg.CGSolver(gemv_variant=-1) as s:
        s.generate_lap2d_matrix(n)
        want = run(s)
    with gpu_pkg.CGSolver(gemv_variant=-1) as s:               # a fresh context: the walk also steps over the side blocks' making
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
        # at least the calls of a call whose side blocks exist (a block made by an earlier, failed attempt stays): the device, the
        # upload, the set-up, per step K1, the step kernel and the copy of v_t, the close, three downloads and the synchronisation;
        # then two uploads, the combine launch, the download and the synchronisation
        assert calls >= 1 + (3 * steps + 7) + 5, calls
        assert _same(got, want)
        assert _same(run(s), want)
        _still_solves(s, n)


# ---- 9. the command line ----------------------------------------------------------------------------------------------------------
def test_cli_apply_prints_the_library_call(gpu_pkg, tmp_path):
    n, steps = 1000, 60
    exe = os.path.join(os.path.dirname(gpu_pkg.cgx.LIB_PATH), "cgsolver")
    out = tmp_path / "times.csv"
    r = subprocess.run([exe, str(n), str(out), "--apply", "invsqrt,%d" % steps], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if "[APPLY]" in ln]
    assert len(lines) == 1, r.stdout
    m = re.search(r"fn = invsqrt, steps = (\d+), steps_done = (\d+), change = (\S+), \|\|x\|\| = (\S+)", lines[0])
    assert m and int(m.group(1)) == steps, lines[0]
    assert out.read_text().startswith("%d,1," % n)
    with gpu_pkg.CGSolver(gemv_variant=-1) as s:
        s.generate_lap2d_matrix(n)
        s.init_source_term(1.0 / n)
        b = s.probe_source_term()
        X, info = s.apply_function(b[None, :], gpu_pkg.cgx.FN_INVSQRT, steps)
    assert int(m.group(2)) == int(info["steps_done"][0])
    assert float(m.group(3)) == pytest.approx(info["change"][0], rel=1e-10)        # printed with 12 digits
    assert float(m.group(4)) == pytest.approx(float(np.linalg.norm(X[0])), rel=1e-10)
