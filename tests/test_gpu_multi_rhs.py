"""cgx_solve_multi / cgx_probe_gemv_multi (csrc/cgx_multi.hip) on the MI355X.

- the plain multi-vector K1 alone: every row of Y and every p.Ap on dense hash matrices against longdouble sums, and on lap2d
  against oracle.gemv;
- every column of a multi solve against oracle.solve of that column alone (fixed iterations and converged);
- columns that break at different iterations, frozen columns, check_every, the alpha safeguard in one column;
- independence: permuted columns, different companions, nrhs = 1 against cgx_solve;
- large n (i * lda past 2^31, and an n where single solves take the symmetric K1) against single solves on the same context;
- no interference with the single path's plan and results; refusals; the fault walk over every HIP call of a multi solve.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 0x3D1F
ERR_BAD_ARG, ERR_HIP, ERR_UNSUPPORTED = 1, 3, 7   # cgx_status (include/cgx.h)


def _diag(n):
    return 1.03 * 2.0 * np.sqrt(n / 3.0)   # dominant diagonal: the hash matrix is SPD (tests/test_gpu_dense_hash.py)


def _rhs_block(oracle, A, n, k, rng_seed=7):
    """k different right-hand sides: the source term, cos(i), seeded random, A x_exact, then scaled variants."""
    rng = np.random.default_rng(rng_seed)
    i = np.arange(n, dtype=np.float64)
    cols = [oracle.init_source_term(n), np.cos(i), rng.standard_normal(n), oracle.gemv(A, rng.standard_normal(n))]
    while len(cols) < k:
        cols.append(rng.standard_normal(n) * (1.0 + len(cols)))
    return np.array(cols[:k])


def _x0_block(n, k):
    X0 = np.zeros((k, n))
    if k > 1:
        X0[1] = np.sin(np.arange(n) * 0.01)   # a nonzero initial guess
    return X0


def _lap2d_solver(pkg, n, **kw):
    s = pkg.CGSolver(gemv_variant=kw.pop("gemv_variant", -1), **kw)
    s.generate_lap2d_matrix(n)
    return s


def _hash_solver(pkg, n, symmetric=True, **kw):
    s = pkg.CGSolver(gemv_variant=kw.pop("gemv_variant", -1), **kw)
    s.generate_lap2d_matrix(n)
    s.probe_fill_matrix_hash(SEED, symmetric=symmetric, diag=_diag(n) if symmetric else 0.0)
    return s


# ---- the plain multi-vector K1 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [257, 384, 511, 512, 289])   # n mod 256 = 1, 128, 255, 0, 33
def test_probe_hash_every_row(gpu_pkg, oracle, n):
    rng = np.random.default_rng(n)
    with _hash_solver(gpu_pkg, n, symmetric=False) as s:
        for k in (1, 2, 3, 8, 16):
            P = rng.standard_normal((k, n))
            Y, pap = s.probe_gemv_multi(P)
            for j in range(k):
                rows, y_ref, abs_ap = oracle.hash_gemv_longdouble(n, SEED, P[j])
                assert oracle.gemv_rows_outside(Y[j][rows], y_ref, abs_ap, n).size == 0, (k, j)
                ref = float(np.sum(P[j].astype(np.longdouble) * y_ref))
                bound = 4e-16 * np.sqrt(n) * float(np.abs(P[j]) @ abs_ap) * 4
                assert abs(pap[j] - ref) <= bound, (k, j, pap[j], ref)


def test_probe_lap2d(gpu_pkg, oracle):
    n = 1000
    A = oracle.generate_lap2d(n)
    rng = np.random.default_rng(3)
    with _lap2d_solver(gpu_pkg, n) as s:
        P = rng.standard_normal((5, n))
        Y, pap = s.probe_gemv_multi(P)
    for j in range(5):
        ref = oracle.gemv(A, P[j])
        assert np.max(np.abs(Y[j] - ref)) <= 1e-13 * np.max(np.abs(ref))
        assert abs(pap[j] - P[j] @ ref) <= 1e-12 * abs(P[j] @ ref)


# ---- every column against the oracle --------------------------------------------------------------------------------------------
def _check_columns(oracle, A, B, X0, X, res, iters, tol):
    for j in range(B.shape[0]):
        xo, ro = oracle.solve(A, B[j], x0=X0[j], max_iter=iters, tol=tol)
        if tol == 0.0:
            assert res[j]["iterations"] == ro["iterations"] == iters, (j, res[j], ro)
            assert np.linalg.norm(X[j] - xo) <= 1e-12 * np.linalg.norm(xo), (j, np.linalg.norm(X[j] - xo) / np.linalg.norm(xo))
        else:
            assert res[j]["converged"] == 1, (j, res[j])
            assert abs(res[j]["iterations"] - ro["iterations"]) <= 0.15 * ro["iterations"] + 1, (j, res[j], ro)
            # ||Ax - b|| / ||b|| after a break on sqrt(r.r) < tol: 1e-11, or what the oracle's own solve of the column reaches
            assert res[j]["rel_residual"] <= max(1e-11, 4.0 * ro["rel_residual"]), (j, res[j], ro)


@pytest.mark.parametrize("n,k,kind", [(64, 3, "lap2d"), (1000, 8, "hash"), (2048, 16, "lap2d"), (4097, 1, "hash"),
                                      (10000, 3, "lap2d")])
def test_fixed_iterations_against_oracle(gpu_pkg, oracle, n, k, kind):
    iters = 12
    A = oracle.generate_lap2d(n) if kind == "lap2d" else oracle.hash_rows(n, 0, n, SEED, True, _diag(n))
    B = _rhs_block(oracle, A, n, k)
    X0 = _x0_block(n, k)
    make = _lap2d_solver if kind == "lap2d" else _hash_solver
    with make(gpu_pkg, n) as s:
        s.set_max_iter(iters)
        s.tolerance(0.0)
        X, res = s.solve_multi(B, X0)
    _check_columns(oracle, A, B, X0, X, res, iters, 0.0)


@pytest.mark.parametrize("n,k,kind", [(64, 16, "lap2d"), (1000, 3, "hash"), (2048, 8, "hash")])
def test_converged_against_oracle(gpu_pkg, oracle, n, k, kind):
    A = oracle.generate_lap2d(n) if kind == "lap2d" else oracle.hash_rows(n, 0, n, SEED, True, _diag(n))
    B = _rhs_block(oracle, A, n, k)
    X0 = _x0_block(n, k)
    make = _lap2d_solver if kind == "lap2d" else _hash_solver
    with make(gpu_pkg, n) as s:
        s.set_max_iter(n)
        s.tolerance(1e-10)
        X, res = s.solve_multi(B, X0)
    _check_columns(oracle, A, B, X0, X, res, n, 1e-10)


# ---- columns that break at different iterations ----------------------------------------------------------------------------------
def test_columns_break_apart(gpu_pkg, oracle):
    n, k = 1000, 4
    A = oracle.generate_lap2d(n)
    B = _rhs_block(oracle, A, n, k)
    x_exact = np.linalg.solve(A, B[0])
    X0 = np.zeros((k, n))
    X0[0] = x_exact
    with _lap2d_solver(gpu_pkg, n) as s:
        s.tolerance(1e-6)
        X, res = s.solve_multi(B, X0)
        assert res[0]["converged"] == 1 and res[0]["iterations"] <= 2, res[0]   # starts next to its solution
        assert all(r["converged"] and r["iterations"] > 5 for r in res[1:]), res
        # frozen columns do not move when the others run longer; check_every changes nothing
        s.tolerance(1e-8)
        s.set_max_iter(40)
        Xa, ra = s.solve_multi(B, X0)
        s.set_max_iter(60)
        Xb, rb = s.solve_multi(B, X0)
        for j in range(k):
            if ra[j]["converged"]:
                assert np.array_equal(Xa[j], Xb[j]) and ra[j]["iterations"] == rb[j]["iterations"], j
    outs = []
    for every in (1, 16, 64):
        with _lap2d_solver(gpu_pkg, n, check_every=every) as s:
            s.tolerance(1e-8)
            Xc, rc = s.solve_multi(B, X0)
            outs.append((Xc, [(r["iterations"], r["converged"], r["residual_prev"], r["residual_last"], r["x_norm"],
                               r["rel_residual"]) for r in rc]))
    for Xc, rc in outs[1:]:
        assert np.array_equal(Xc, outs[0][0]) and rc == outs[0][1]


def test_zero_initial_residual_breaks_at_zero(gpu_pkg, oracle):
    n = 500
    A = oracle.generate_lap2d(n)
    B = _rhs_block(oracle, A, n, 3)
    X0 = np.zeros((3, n))
    X0[1] = np.linalg.solve(A, B[1])
    B[1] = A @ X0[1]
    with _lap2d_solver(gpu_pkg, n) as s:
        s.tolerance(1e-6)
        X, res = s.solve_multi(B, X0)
    # r0 = b - A x0 is tiny: the column breaks at iteration 0, after its first update (cg.cc:120-121), the others run on
    xo, ro = oracle.solve(A, B[1], x0=X0[1], max_iter=n, tol=1e-6)
    assert res[1]["iterations"] == ro["iterations"] == 0 and res[1]["converged"] == 1
    assert np.linalg.norm(X[1] - xo) <= 1e-12 * np.linalg.norm(xo)
    assert res[0]["iterations"] > 5 and res[2]["iterations"] > 5


def test_alpha_safeguard_in_one_column(gpu_pkg, oracle):
    """tol = 0 and a zero right-hand side: that column's alpha is 0/0 = NaN (the single path's behaviour), the others are clean."""
    n, k = 300, 3
    A = oracle.generate_lap2d(n)
    B = _rhs_block(oracle, A, n, k)
    B[1] = 0.0
    with _lap2d_solver(gpu_pkg, n) as s:
        s.set_max_iter(5)
        s.tolerance(0.0)
        X, res = s.solve_multi(B)
        x1 = np.zeros(n)
        s.set_source_term(B[1])
        r1 = s.solve(x1)
    assert np.isnan(X[1]).all() and np.isnan(x1).all() and np.isnan(res[1]["x_norm"]) == np.isnan(r1["x_norm"])
    _check_columns(oracle, A, B[[0, 2]], np.zeros((2, n)), X[[0, 2]], [res[0], res[2]], 5, 0.0)


# ---- independence --------------------------------------------------------------------------------------------------------------
def test_permutation_and_companions_bitwise(gpu_pkg, oracle):
    n, k = 1500, 8
    A = oracle.hash_rows(n, 0, n, SEED, True, _diag(n))
    B = _rhs_block(oracle, A, n, k)
    X0 = _x0_block(n, k)
    perm = np.random.default_rng(1).permutation(k)
    with _hash_solver(gpu_pkg, n) as s:
        s.tolerance(1e-9)
        X, res = s.solve_multi(B, X0)
        Xp, resp = s.solve_multi(B[perm], X0[perm])
        B2 = B.copy()
        B2[1:] = B2[1:][::-1] * 3.0          # column 0 among different companions, same k
        X2, res2 = s.solve_multi(B2, X0)
    assert np.array_equal(Xp, X[perm])
    assert [resp[j]["iterations"] for j in range(k)] == [res[p]["iterations"] for p in perm]
    assert [resp[j]["residual_prev"] for j in range(k)] == [res[p]["residual_prev"] for p in perm]
    assert np.array_equal(X2[0], X[0]) and res2[0]["residual_prev"] == res[0]["residual_prev"]


def test_one_rhs_matches_single_solve(gpu_pkg, oracle):
    n = 2048
    with _lap2d_solver(gpu_pkg, n) as s:
        s.init_source_term(1.0 / n)
        b = oracle.init_source_term(n)   # bit-identical to the library's (cgx_init_source_term)
        x = np.zeros(n)
        r = s.solve(x)
        X, res = s.solve_multi(b[None, :])
    assert res[0]["iterations"] == r["iterations"]
    assert np.linalg.norm(X[0] - x) <= 1e-12 * np.linalg.norm(x)


# ---- large n against single solves on the same context ----------------------------------------------------------------------------
def _against_single(s, B, iters):
    s.set_max_iter(iters)
    s.tolerance(0.0)
    X, res = s.solve_multi(B)
    for j in range(B.shape[0]):
        s.set_source_term(B[j])
        x = np.zeros(B.shape[1])
        r = s.solve(x)
        assert res[j]["iterations"] == r["iterations"] == iters
        assert np.linalg.norm(X[j] - x) <= 1e-12 * np.linalg.norm(x), (j, np.linalg.norm(X[j] - x) / np.linalg.norm(x))


@pytest.mark.parametrize("n,k", [(32768, 8), (46341, 3)])
def test_large_n_against_single(gpu_pkg, n, k):
    rng = np.random.default_rng(n)
    with _lap2d_solver(gpu_pkg, n, gemv_variant=0) as s:
        plan = s.gemv_plan()
        _against_single(s, rng.standard_normal((k, n)), 3)
        assert s.gemv_plan() == plan


def test_symmetric_plan_unchanged(gpu_pkg):
    n = 16640
    rng = np.random.default_rng(5)
    with _hash_solver(gpu_pkg, n, gemv_variant=0) as s:
        plan = s.gemv_plan()
        assert plan["variant"] == 6, plan
        _against_single(s, rng.standard_normal((2, n)), 3)
        assert s.gemv_plan() == plan


# ---- no interference with the single path ------------------------------------------------------------------------------------
@pytest.mark.parametrize("resident", [True, False])
def test_single_multi_single(gpu_pkg, oracle, monkeypatch, resident):
    n = 2048
    if resident:
        monkeypatch.delenv("CGX_RESIDENT", raising=False)
    with gpu_pkg.CGSolver(gemv_variant=0 if resident else -1) as s:
        s.generate_lap2d_matrix(n)
        s.init_source_term(1.0 / n)
        s.set_max_iter(200)
        plan = s.gemv_plan()
        assert (plan["variant"] == 4) == resident, plan
        x1 = np.zeros(n)
        r1 = s.solve(x1)
        B = _rhs_block(oracle, oracle.generate_lap2d(n), n, 5)
        s.solve_multi(B)
        assert s.gemv_plan() == plan
        x2 = np.zeros(n)
        r2 = s.solve(x2)
    assert np.array_equal(x1, x2)
    for key in ("iterations", "converged", "residual_prev", "residual_last", "x_norm", "rel_residual"):
        assert r1[key] == r2[key], key


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals(gpu_pkg, oracle):
    cgx = gpu_pkg.cgx
    n = 256
    B = np.ones((2, n))
    with gpu_pkg.CGSolver(comm_mode=cgx.COMM_LOOPBACK, nranks=2, gemv_variant=-1) as s:
        s.generate_lap2d_matrix(n)
        with pytest.raises(cgx.CgxError) as e:
            s.solve_multi(B)
        assert e.value.status == ERR_UNSUPPORTED
    with gpu_pkg.CGSolver(matrix_format=cgx.MATRIX_BANDED, gemv_variant=-1) as s:
        s.generate_lap2d_matrix(n)
        with pytest.raises(cgx.CgxError) as e:
            s.solve_multi(B)
        assert e.value.status == ERR_UNSUPPORTED
    with _lap2d_solver(gpu_pkg, n) as s:
        for bad in (np.ones((0, n)), np.ones((17, n))):
            with pytest.raises(cgx.CgxError) as e:
                s.solve_multi(bad)
            assert e.value.status == ERR_BAD_ARG
        Bs = np.ones((2, n))
        Xs = np.zeros((2, n))
        rc = cgx.lib().cgx_solve_multi(s._h, 2, cgx._dp(Bs), n - 1, cgx._dp(Xs), n, None)
        assert rc == ERR_BAD_ARG
        X, res = s.solve_multi(_rhs_block(oracle, oracle.generate_lap2d(n), n, 2))
        assert all(r["converged"] for r in res)


# ---- fault walk -----------------------------------------------------------------------------------------------------------------
def test_fault_walk(gpu_pkg, oracle):
    import torch
    cgx = gpu_pkg.cgx
    n = 600
    A = oracle.generate_lap2d(n)
    B = _rhs_block(oracle, A, n, 3)
    with _lap2d_solver(gpu_pkg, n) as s:
        s.set_max_iter(40)
        X_ref, res_ref = s.solve_multi(B)
        free0 = torch.cuda.mem_get_info()[0]
        calls = 0
        while True:
            s._set_fault_after(calls)
            try:
                X, res = s.solve_multi(B)
            except cgx.CgxError as e:
                assert e.status == ERR_HIP, (calls, e)
                assert torch.cuda.mem_get_info()[0] == free0, calls
                calls += 1
                assert calls < 500
                continue
            s._set_fault_after(-1)
            break
        assert calls > 10
        X2, res2 = s.solve_multi(B)
    assert np.array_equal(X2, X_ref) and np.array_equal(X, X_ref)
    assert [r["residual_prev"] for r in res2] == [r["residual_prev"] for r in res_ref]
