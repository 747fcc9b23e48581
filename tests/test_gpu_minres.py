"""cgx_solve_minres (csrc/cgx_minres.hip, csrc/cgx_minres_host.cpp) on the MI355X: MINRES, (A + sigma I) x = b for up to 16 shifts of
either sign on one Lanczos recurrence, A symmetric and not necessarily definite.

- every shift against tests/minres_reference.py (pinned on the CPU by tests/test_minres_abi.py) at fixed iterations and converged:
  dense, the symmetric K1, CSR at 1, 8 and 64 lanes per row; what every shift reports against the reference and a host
  recomputation; the converged solutions against np.linalg.solve;
- independence of the other shifts, their number (the kernel width), their order and check_every, bit for bit;
- the Lanczos breakdown and shifts that are singular on the Krylov space;
- vectors above 262144 rows and the symmetric K1's partial layout;
- no interference with the single, the multi and the shifted path; refusals; the fault walk over every HIP call; the CLI.
tests/test_gpu_minres_edges.py goes on from here: the ends of the loop, launch 0, every width above 262144 rows, 257 and more K1
partials, ldx > n.

The bars are the project's own (tests/test_gpu_shifted.py): 1e-12 on x and x_norm, 1e-9 on reported residuals, _check_rel_residual
of tests/test_gpu_jacobi_scaled.py on rel_residual.  tests/test_minres_abi.py shows the reference's float64 and long-double runs
3e-15 apart at 12 iterations, so 1e-12 leaves room for another summation order and none for a wrong rotation.
"""
import os
import subprocess

import numpy as np
import pytest

import long_vector_reference as lv
import minres_reference as mr
import test_gpu_csr as tc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x3D1F
ERR_BAD_ARG, ERR_HIP, ERR_UNSUPPORTED = 1, 3, 7   # cgx_status (include/cgx.h)
SHIFT_X_BOUND, RESIDUAL_BOUND, NORM_BOUND = 1e-12, 1e-9, 1e-12
KEYS = ("iterations", "converged", "residual_prev", "residual_last", "x_norm", "rel_residual")
S_ALT = [0.0, 1.0, -1.0, 50.0, -50.0, 1e4]

_cache = {}


def _problem(oracle, kind, n):
    """(A, b, shifts) of a test problem, made once.  lap2d: the generator's matrix and source term; hash0: the symmetric hash matrix
    with a zero diagonal (indefinite by itself, spectrum about +-26) and cos(i); althash: its rows with the diagonal replaced by
    +-4r alternating, r = 2 sqrt(n / 3) (256 negative eigenvalues at n = 513, |lambda| in [87, 124]); diag5: diag(1, 2, 3, -4, -5
    cycling) and ones (a Krylov space of dimension 5)."""
    key = ("problem", kind, n)
    if key not in _cache:
        if kind == "lap2d":
            A, b = oracle.generate_lap2d(n), oracle.init_source_term(n)
        elif kind == "diag5":
            A, b = np.diag(np.array([1.0, 2.0, 3.0, -4.0, -5.0])[np.arange(n) % 5]), np.ones(n)
        else:
            A, b = oracle.hash_rows(n, 0, n, SEED, True, 0.0), np.cos(np.arange(n, dtype=np.float64))
            if kind == "althash":
                A = A.copy()
                A[np.arange(n), np.arange(n)] = 4.0 * 2.0 * np.sqrt(n / 3.0) * np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
        if kind in ("lap2d", "hash0"):
            ev = np.linalg.eigvalsh(A)   # two interior shifts at the midpoints of eigenvalues 3|4 and n-5|n-4, one beyond the spectrum
            S = [0.0, 1e-3, 1.0, 100.0, -0.5 * (ev[3] + ev[4]), -0.5 * (ev[n - 5] + ev[n - 4]), -(ev[-1] + 5.0), -1e4]
        else:
            S = list(S_ALT)
        A.setflags(write=False)
        b.setflags(write=False)
        _cache[key] = (A, b, S)
    return _cache[key]


def _reference(oracle, kind, n, shifts, max_iter, tol):
    """minres_reference.minres on a test problem in float64, computed once and shared."""
    key = ("ref", kind, n, tuple(shifts), max_iter, tol)
    if key not in _cache:
        A, b, _ = _problem(oracle, kind, n)
        _cache[key] = mr.minres(A, b, shifts, max_iter, tol)
        for q in _cache[key]:
            q["x"].setflags(write=False)
    return _cache[key]


def _solver(pkg, oracle, kind, n, storage="dense", **kw):
    fmt = pkg.MATRIX_CSR if storage == "csr" else pkg.MATRIX_DENSE
    s = pkg.CGSolver(gemv_variant=kw.pop("gemv_variant", -1), matrix_format=fmt, **kw)
    A, b, _ = _problem(oracle, kind, n)
    if kind == "lap2d":
        s.generate_lap2d_matrix(n)
        s.init_source_term(1.0 / n)
        return s
    if storage == "csr":
        if kind == "diag5":
            s.set_matrix_csr(np.arange(n + 1), np.arange(n), np.diag(A).copy(), n)   # one entry per row
        else:
            s.set_matrix_csr(*tc.dense_to_csr(A), n)                                 # full rows
    elif kind == "hash0":
        s.generate_lap2d_matrix(n)
        s.probe_fill_matrix_hash(SEED, symmetric=True, diag=0.0)
    else:
        s.set_matrix_dense(A)
    s.set_source_term(b)
    return s


def _tuples(res):
    return [tuple(r[k] for k in KEYS) for r in res]


def _check_against_reference(X, res, ref, A_times, absA_times, b, shifts, iters, row_entries, what):
    """The bars of a fixed-iteration run: x, both reported residuals, x_norm and rel_residual of every shift, and iterations and
    converged exactly: (iters, 0), or with iters = None what the reference reports for the shift."""
    from test_gpu_jacobi_scaled import _check_rel_residual
    for j, sigma in enumerate(shifts):
        q = ref[j]
        err = np.linalg.norm(X[j] - q["x"]) / np.linalg.norm(q["x"])
        xn = float(np.linalg.norm(X[j]))
        offs = {k: abs(res[j][k] - q[k]) / q[k] for k in ("residual_prev", "residual_last")}
        print("%s sigma=%g: iterations %d, |dx|/|x| = %.2e, residual_prev off by %.2e, residual_last by %.2e, x_norm by %.2e" % (
            what, sigma, res[j]["iterations"], err, offs["residual_prev"], offs["residual_last"], abs(res[j]["x_norm"] - xn) / xn))
        want = (q["iterations"], q["converged"])       # iters = None: shifts freeze on the way, each as the reference says
        assert (res[j]["iterations"], res[j]["converged"]) == want and (iters is None or want == (iters, 0)), (sigma, res[j], q)
        assert err <= SHIFT_X_BOUND, (sigma, err)
        for k, off in offs.items():
            assert off <= RESIDUAL_BOUND, (sigma, k, res[j][k], q[k])
        assert abs(res[j]["x_norm"] - xn) <= NORM_BOUND * xn, (sigma, res[j]["x_norm"], xn)
        assert res[j]["residual_last"] <= res[j]["residual_prev"]   # MINRES: the residual norm never grows
        _check_rel_residual(res[j], A_times(X[j]) + sigma * X[j], absA_times(np.abs(X[j])) + abs(sigma) * np.abs(X[j]), b, row_entries,
                            (what, sigma))


# ---- 1. fixed iterations against the reference ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n,storage,variant", [("lap2d", 64, "dense", -1), ("lap2d", 257, "dense", -1), ("lap2d", 511, "dense", -1),
                                                    ("lap2d", 1000, "dense", -1), ("hash0", 513, "dense", -1),
                                                    ("lap2d", 1000, "csr", -1), ("lap2d", 1000, "csr", 70008)])
def test_fixed_iterations_against_reference(gpu_pkg, oracle, kind, n, storage, variant):
    iters = 12
    A, b, S = _problem(oracle, kind, n)
    with _solver(gpu_pkg, oracle, kind, n, storage, gemv_variant=variant) as s:
        plan = s.gemv_plan()
        assert (plan["variant"] == 7) == (storage == "csr"), plan
        if variant == 70008:
            assert plan["R"] == 8, plan
        s.set_max_iter(iters)
        s.tolerance(0.0)
        X, res = s.solve_minres(S)
        assert s.gemv_plan() == plan
    assert X.shape == (len(S), n)
    absA = np.abs(A)
    _check_against_reference(X, res, _reference(oracle, kind, n, S, iters, 0.0), lambda x: A @ x, lambda x: absA @ x, b, S, iters,
                             6 if kind == "lap2d" else n, "fixed %s n=%d %s %d" % (kind, n, storage, variant))
    assert all(r["gemv_bytes"] > 0 and r["seconds_loop"] > 0 and r["gemv_ms_avg"] == 0 for r in res), res[0]


# ---- 2. converged -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n,storage", [("lap2d", 64, "dense"), ("lap2d", 257, "dense"), ("lap2d", 1000, "dense"),
                                            ("althash", 513, "dense"), ("althash", 513, "csr")])
def test_converged_against_reference(gpu_pkg, oracle, kind, n, storage):
    """The bars of tests/test_gpu_shifted.py test_converged_against_oracle against the float64 reference, and for every shift
    ||x - x*|| / ||x*|| <= 2 kappa(A + sigma I) rel_residual + 1e-13 kappa against np.linalg.solve: the standard bound plus the
    host solve's own rounding.  Interior shifts of the dense part of a spectrum do not converge without reorthogonalisation and
    are not in the lists."""
    tol = 1e-10
    A, b, S = _problem(oracle, kind, n)
    with _solver(gpu_pkg, oracle, kind, n, storage) as s:
        if storage == "csr":
            plan = s.gemv_plan()
            assert plan["variant"] == 7 and plan["R"] == 64, plan   # full rows: 64 lanes per row
        s.set_max_iter(n)
        s.tolerance(tol)
        X, res = s.solve_minres(S)
    ref = _reference(oracle, kind, n, S, n, tol)
    nb = np.linalg.norm(b)
    for j, sigma in enumerate(S):
        q = ref[j]
        As = A + sigma * np.eye(n)
        q_rel = float(np.linalg.norm(As @ q["x"] - b) / nb)
        xs = np.linalg.solve(As, b)
        kappa = np.linalg.cond(As)
        err = np.linalg.norm(X[j] - xs) / np.linalg.norm(xs)
        print("converged %s n=%d %s sigma=%g: iterations %d (reference %d), rel_residual %.3e (reference %.3e), error %.2e, kappa %.2e" % (
            kind, n, storage, sigma, res[j]["iterations"], q["iterations"], res[j]["rel_residual"], q_rel, err, kappa))
        assert q["converged"] == 1 and res[j]["converged"] == 1, (sigma, res[j], q)
        assert abs(res[j]["iterations"] - q["iterations"]) <= 0.15 * q["iterations"] + 1, (sigma, res[j], q)
        assert res[j]["rel_residual"] <= max(1e-11, 4.0 * q_rel), (sigma, res[j], q_rel)
        assert res[j]["residual_last"] < tol <= res[j]["residual_prev"], (sigma, res[j])
        assert err <= 2.0 * kappa * res[j]["rel_residual"] + 1e-13 * kappa, (sigma, err, kappa)


# ---- 3. independence, bit for bit -----------------------------------------------------------------------------------------------------
def test_independent_of_companions_width_order_and_poll(gpu_pkg, oracle):
    """40 iterations at tol 1e-8: the large shifts freeze on the way and stay frozen, the others run to the end."""
    n = 1000
    _, _, S = _problem(oracle, "lap2d", n)
    S8 = [S[0], -1.0] + S[2:]                               # 8 shifts: width 8
    others = [0.0, 0.5, -0.5, 2.0, -2.5, 3.0, -3.5, 8.0, -9.0, 10.0, -20.0, 50.0, 200.0, -1e3, 1e5]   # 15 other shifts
    perm = np.random.default_rng(1).permutation(len(S8))
    outs = []
    for every in (1, 7, None):
        kw = {} if every is None else {"check_every": every}
        with _solver(gpu_pkg, oracle, "lap2d", n, **kw) as s:
            s.set_max_iter(40)
            s.tolerance(1e-8)
            X, res = s.solve_minres(S8)
            outs.append((X, _tuples(res)))
            if every is None:
                Xp, resp = s.solve_minres([S8[p] for p in perm])
                X1, res1 = s.solve_minres([-1.0])                               # width 1
                X16, res16 = s.solve_minres(others[:7] + [-1.0] + others[7:])   # width 16
                X2, res2 = s.solve_minres([-1.0, -1.0])                         # shifts may repeat
    X, t = outs[-1]
    its = [q[0] for q in t]
    print("independence: iterations", its, "converged", [q[1] for q in t])
    assert 0 < min(its) < max(its) == 40 and any(q[1] for q in t) and not all(q[1] for q in t), t
    for Xe, te in outs[:-1]:
        assert np.array_equal(Xe, X) and te == t
    assert np.array_equal(Xp, X[perm]) and _tuples(resp) == [t[p] for p in perm]
    assert np.array_equal(X1[0], X[1]) and np.array_equal(X16[7], X[1]) and np.array_equal(X2[0], X[1]) and np.array_equal(X2[1], X[1])
    assert _tuples(res1)[0] == t[1] == _tuples(res16)[7] == _tuples(res2)[0] == _tuples(res2)[1]


# ---- 4. breakdown and singular shifts -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", ["dense", "csr"])
def test_breakdown_and_singular_shifts(gpu_pkg, oracle, storage):
    """diag(1, 2, 3, -4, -5 cycling), b = ones: the recurrence breaks down in step 4 (beta_5 of a few 1e-15 against a threshold of
    about 7e-11).  sigma = 0 and 0.5 end there with the exact solution; sigma = 4 and -2 are exactly singular (|gamma bar| of the
    order 1e-15 against 2.07 for sigma = 0.5) and leave the regular shifts' bits alone."""
    n = 600
    A, b, _ = _problem(oracle, "diag5", n)
    d = np.diag(A)
    with _solver(gpu_pkg, oracle, "diag5", n, storage) as s:
        if storage == "csr":
            assert s.gemv_plan()["R"] == 1, s.gemv_plan()
        s.set_max_iter(n)
        s.tolerance(0.0)
        X, res = s.solve_minres([0.0, 0.5])
        X4, res4 = s.solve_minres([4.0, 0.0, -2.0, 0.5])
    for j, sigma in enumerate([0.0, 0.5]):
        err = np.abs(X[j] - 1.0 / (d + sigma)).max()
        print("breakdown %s sigma=%g: %r, max error %.2e" % (storage, sigma, _tuples(res)[j][:4], err))
        assert (res[j]["iterations"], res[j]["converged"], res[j]["residual_last"]) == (4, 1, 0.0), res[j]
        assert err <= 1e-13, (sigma, err)
    for j in (0, 2):
        assert (res4[j]["iterations"], res4[j]["converged"]) == (4, 0) and np.isfinite(X4[j]).all(), res4[j]
        assert all(np.isfinite(res4[j][k]) for k in KEYS), res4[j]
    assert np.array_equal(X4[1], X[0]) and np.array_equal(X4[3], X[1])
    assert [_tuples(res4)[1], _tuples(res4)[3]] == _tuples(res)


# ---- 5. larger shapes -----------------------------------------------------------------------------------------------------------------
def test_long_vectors_csr(gpu_pkg):
    """263501 rows: workgroups 0 - 5 of the step kernel take a second trip of the striding loop, and the last tile is ragged."""
    n, iters = lv.N_LONG, 12
    S = [0.0, 1.0, -1.0, 100.0, -3.7, -20.0, -1e4]
    csr = tc.lap2d_csr(n)
    b = lv.normal_b(n)
    with gpu_pkg.CGSolver(gemv_variant=-1, matrix_format=gpu_pkg.MATRIX_CSR) as s:
        s.generate_lap2d_matrix(n)
        s.set_source_term(b)
        assert s.gemv_plan()["variant"] == 7, s.gemv_plan()
        s.set_max_iter(iters)
        s.tolerance(0.0)
        X, res = s.solve_minres(S)
    ref = mr.minres(csr, b, S, iters, 0.0)
    absdata = np.abs(csr[2])
    _check_against_reference(X, res, ref, lambda x: lv.matvec(csr[0], csr[1], csr[2], x), lambda x: lv.matvec(csr[0], csr[1], absdata, x),
                             b, S, iters, 6, "long csr n=%d" % n)


def test_symmetric_k1(gpu_pkg, oracle):
    """n = 16640, the smallest size that takes the symmetric upper-triangle K1 (its partial count and tail differ): 3 iterations,
    one shift of each sign, against the reference with the products made in row chunks."""
    n, iters, chunk = 16640, 3, 2080
    S = [7.5, -7.5]
    b = np.cos(np.arange(n, dtype=np.float64))

    def rows():
        for r0 in range(0, n, chunk):
            yield r0, oracle.hash_rows(n, r0, chunk, SEED, True, 0.0)

    def times(x):
        y = np.empty(n)
        for r0, R in rows():
            y[r0:r0 + chunk] = R @ x
        return y

    with gpu_pkg.CGSolver(gemv_variant=0) as s:
        s.generate_lap2d_matrix(n)
        s.probe_fill_matrix_hash(SEED, symmetric=True, diag=0.0)
        s.set_source_term(b)
        plan = s.gemv_plan()
        assert plan["variant"] == 6, plan
        s.set_max_iter(iters)
        s.tolerance(0.0)
        X, res = s.solve_minres(S)
        assert s.gemv_plan() == plan
    ref = mr.minres(times, b, S, iters, 0.0)
    AX, AAX = np.empty((2, n)), np.empty((2, n))           # both shifts' products from one pass over the rows
    for r0, R in rows():
        AX[:, r0:r0 + chunk] = X @ R.T
        AAX[:, r0:r0 + chunk] = np.abs(X) @ np.abs(R).T
    for j, sigma in enumerate(S):
        _check_against_reference(X[j:j + 1], res[j:j + 1], ref[j:j + 1], lambda x, j=j: AX[j], lambda x, j=j: AAX[j], b, [sigma], iters, n,
                                 "symmetric K1 n=%d" % n)


# ---- 6. no interference with the other solve paths ------------------------------------------------------------------------------------
@pytest.mark.parametrize("resident", [True, False])
def test_no_interference(gpu_pkg, monkeypatch, resident):
    n = 2048
    if resident:
        monkeypatch.delenv("CGX_RESIDENT", raising=False)
    B = np.array([np.cos(np.arange(n) * 0.5), np.sin(np.arange(n) * 0.25) + 1.0])
    with gpu_pkg.CGSolver(gemv_variant=0 if resident else -1) as s:
        s.generate_lap2d_matrix(n)
        s.init_source_term(1.0 / n)
        s.set_max_iter(200)
        plan = s.gemv_plan()
        assert (plan["variant"] == 4) == resident, plan

        def round_of_three():
            x = np.zeros(n)
            r = s.solve(x)
            Xm, rm = s.solve_multi(B)
            Xs, rs = s.solve_shifted([0.0, 1.0, 50.0])
            return x, tuple(r[k] for k in KEYS), Xm, _tuples(rm), Xs, _tuples(rs)

        first = round_of_three()
        X, res = s.solve_minres([0.0, -1.0, 50.0, -50.0])
        assert s.gemv_plan() == plan
        second = round_of_three()
        assert s.gemv_plan() == plan
        X2, res2 = s.solve_minres([0.0, -1.0, 50.0, -50.0])
    for a, b in zip(first, second):
        assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b
    assert np.array_equal(X, X2) and _tuples(res) == _tuples(res2)
    assert np.isfinite(X).all() and all(res[j]["converged"] == 1 and res[j]["iterations"] < 30 for j in (2, 3)), res
    if resident:   # the per-launch K1 under a persistent plan: the bits of a context that never had one
        with gpu_pkg.CGSolver(gemv_variant=-1) as s:
            s.generate_lap2d_matrix(n)
            s.init_source_term(1.0 / n)
            s.set_max_iter(200)
            Xr, resr = s.solve_minres([0.0, -1.0, 50.0, -50.0])
        assert np.array_equal(X, Xr) and _tuples(res) == _tuples(resr)


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------------
def _refused(s, cgx, status, shifts=(0.0, -1.0)):
    with pytest.raises(cgx.CgxError) as e:
        s.solve_minres(list(shifts))
    assert e.value.status == status, e.value
    return str(e.value)


def test_refusals(gpu_pkg, monkeypatch):
    cgx = gpu_pkg.cgx
    n = 256
    with gpu_pkg.CGSolver(comm_mode=cgx.COMM_LOOPBACK, nranks=2, gemv_variant=-1) as s:
        s.generate_lap2d_matrix(n)
        s.init_source_term(1.0 / n)
        _refused(s, cgx, ERR_UNSUPPORTED)
        assert s.solve(np.zeros(n))["converged"] == 1   # the context is still good for what it was made for
    with gpu_pkg.CGSolver(matrix_format=cgx.MATRIX_BANDED, gemv_variant=-1) as s:
        s.generate_lap2d_matrix(n)
        s.init_source_term(1.0 / n)
        _refused(s, cgx, ERR_UNSUPPORTED)
        assert s.solve(np.zeros(n))["converged"] == 1
    monkeypatch.delenv("CGX_RESIDENT", raising=False)
    for variant in (40000, 50000):
        with gpu_pkg.CGSolver(gemv_variant=variant) as s:
            s.generate_lap2d_matrix(1024)
            s.init_source_term(1.0 / 1024)
            _refused(s, cgx, ERR_UNSUPPORTED)
            assert s.solve(np.zeros(1024))["converged"] == 1
    with gpu_pkg.CGSolver(gemv_variant=-1) as s:
        L = cgx.lib()
        sig = np.array([0.0, -1.0])
        Xs = np.full((2, n), 7.0)
        assert L.cgx_solve_minres(s._h, 2, cgx._dp(sig), cgx._dp(Xs), n, None) == ERR_BAD_ARG   # no matrix yet
        s.generate_lap2d_matrix(n)
        _refused(s, cgx, ERR_BAD_ARG)                       # no source term yet
        s.init_source_term(1.0 / n)
        s.set_preconditioner("jacobi")
        assert "ignored" in _refused(s, cgx, ERR_UNSUPPORTED)
        s.set_preconditioner(None)
        X, res = s.solve_minres([0.0, -1.0])
        assert all(r["converged"] for r in res)
        _refused(s, cgx, ERR_BAD_ARG, shifts=())
        _refused(s, cgx, ERR_BAD_ARG, shifts=[1.0] * 17)
        assert "shift 1" in _refused(s, cgx, ERR_BAD_ARG, shifts=[0.0, float("nan")])
        assert "shift 2" in _refused(s, cgx, ERR_BAD_ARG, shifts=[0.0, -1.0, float("-inf")])
        _refused(s, cgx, ERR_BAD_ARG, shifts=[float("inf")])
        assert L.cgx_solve_minres(s._h, 2, cgx._dp(sig), cgx._dp(Xs), n - 1, None) == ERR_BAD_ARG
        assert L.cgx_solve_minres(s._h, 2, None, cgx._dp(Xs), n, None) == ERR_BAD_ARG
        assert L.cgx_solve_minres(s._h, 2, cgx._dp(sig), None, n, None) == ERR_BAD_ARG
        s.solve_begin(np.zeros(n))
        _refused(s, cgx, ERR_BAD_ARG)                       # an open begin / end pair
        s.solve_end()
        assert (Xs == 7.0).all()                            # X is written only when the call succeeds
        X2, res2 = s.solve_minres([0.0, -1.0])              # after every refusal a valid call succeeds, with the same bits
        assert np.array_equal(X2, X) and _tuples(res2) == _tuples(res)
        assert L.cgx_solve_minres(s._h, 2, cgx._dp(sig), cgx._dp(Xs), n, None) == 0   # res may be NULL
        assert np.array_equal(Xs, X)
        assert s.solve(np.zeros(n))["converged"] == 1


# ---- 8. injected host-side errors -----------------------------------------------------------------------------------------------------
def test_fault_walk(gpu_pkg):
    """cgx_probe_set_fault_after: the N-th runtime call of the solve is not made and reports failure (no GPU fault occurs).  Every
    step of the walk returns CGX_ERR_HIP, leaves X untouched and no memory behind, and the context solves afterwards."""
    import torch
    cgx = gpu_pkg.cgx
    n = 300
    sig = np.array([0.0, -2.0])
    with gpu_pkg.CGSolver(gemv_variant=-1) as s:
        s.generate_lap2d_matrix(n)
        s.init_source_term(1.0 / n)
        s.set_max_iter(3)
        s.tolerance(0.0)
        X_ref, res_ref = s.solve_minres(sig)
        free0 = torch.cuda.mem_get_info()[0]
        L = cgx.lib()
        calls = 0
        while True:
            Xw = np.full((2, n), 7.0)
            s._set_fault_after(calls)
            st = L.cgx_solve_minres(s._h, 2, cgx._dp(sig), cgx._dp(Xw), n, None)
            if st == 0:
                s._set_fault_after(-1)
                break
            assert st == ERR_HIP, (calls, st)
            assert (Xw == 7.0).all(), calls
            assert torch.cuda.mem_get_info()[0] == free0, calls
            calls += 1
            assert calls < 200
        print("fault walk: %d runtime calls" % calls)
        assert calls > 10
        X2, res2 = s.solve_minres(sig)
        assert s.solve(np.zeros(n))["iterations"] == 3
    assert np.array_equal(X2, X_ref) and np.array_equal(Xw, X_ref)
    assert _tuples(res2) == _tuples(res_ref)


# ---- 9. the command line --------------------------------------------------------------------------------------------------------------
def test_cli_minres(gpu_pkg, mtx_path, tmp_path):
    exe = os.path.join(ROOT, "conjugate-gradient_amd", "cgsolver")
    out = tmp_path / "out.csv"
    for extra in ([], ["--csr"]):
        r = subprocess.run([exe, mtx_path, str(out), "--minres", "0,1,-100"] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.stdout, r.stderr)
        lines = [ln for ln in r.stdout.splitlines() if "[SHIFT" in ln]
        assert len(lines) == 3, r.stdout
        its = [int(ln.split("iterations = ")[1].split(",")[0]) for ln in lines]
        assert its[0] > its[1] > its[2] > 0, lines
        assert all("converged = 1" in ln for ln in lines), lines
    assert out.read_text().startswith("10000,1,")
    r = subprocess.run([exe, mtx_path, str(out), "--minres", "0,-1", "--jacobi"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "preconditioner" in r.stderr, (r.stdout, r.stderr)
