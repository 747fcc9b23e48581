"""cgx_solve_minres (csrc/cgx_minres.hip, csrc/cgx_minres_host.cpp) where tests/test_gpu_minres.py does not look: the ends of the
loop, launch 0, the striding trip at every width, more than 256 K1 partials, ldx > n and a context that changes its problem.

That module reaches k_minres_close only with every shift running and no breakdown, launch 0 only with a finite nonzero b, the
striding trip of k_minres_step<W> (rows above 256 * 1024) only at W = 8 with every shift running, and dense storage only up to
n = 1000: 250 K1 partials (the general K1 runs 4 rows per workgroup from n = 512), so that fold_pap (csrc/cgx_device.h: four
clamped loads per thread at f + 256 u, then steps of 1024) never left its first slot, and 4 tiles of 256 rows.  Here, each case at
the smallest n that reaches its path:

  case  problem                      path
  A1    diag5 n = 600 (the existing  max_iter = 5: launches 0 .. 4 close columns 0 .. 3, so column 4 and the breakdown behind it
        breakdown problem), dense    (beta_5 of a few 1e-15) fall to k_minres_close, its singular rule included; max_iter = 4: the
        and CSR at one lane          close kernel's plain branch beside them; max_iter = 0: its k == 0 branch, and b = 0 there,
                                     which no launch sees (the host reports it converged)
  A2    lap2d n = 257 dense, tol     max_iter = m + 1 for a shift the long run froze at m: |phibar| < tol in the last column, the
        1e-10, six shifts            conv branch of k_minres_close; max_iter = m: the same column never closed; check_every = 1
  A3    hash0 n = 513 dense, lap2d   launch 0: b = 0 (ww == 0: conv = 1 at column 0), a b that is not finite (frozen unconverged,
        n = 1000 CSR                 and nothing of it may outlive the solve); sigma = +-1e200: gamma overflows in column 0, the
                                     `finite` rule, beside two running shifts (n as in test_fixed_iterations_against_reference)
  A4    lap2d and diag5 as CSR,      lv.N_LONG, the project's smallest n with a second striding trip (workgroups 0 .. 5) and a
        n = 263501                   ragged last tile: W = 16 with 8 shifts freezing in columns 2 .. 9 (predicated stores, the
                                     re-loads of d1p / d2p / X), W = 1, 2, 4 bit for bit, the breakdown in the step and in the
                                     close kernel
  A5    hash0 dense n = 1028, 2052,  257 K1 partials (one in slot 1 of fold_pap), 513 (one in slot 2), 1025 (one in a second
        4100                         trip); 5, 9 and 17 row tiles, the last with 4 rows
  A6    lap2d n = 257 / 1000 dense   hipMemcpy2D at ldx = n + 5; free_problem and ensure_side_block between three problems

Everything is judged by tests/minres_reference.py (pinned on these scenarios by tests/test_minres_abi.py, float64 against long
double at most 4.7e-15 apart in x) under the bars of tests/test_gpu_minres.py, unchanged: 1e-12 on x, 1e-9 on the reported
residuals, iterations and converged exactly.  Where two runs must agree they agree bit for bit.  Every reference is computed here,
once, and the time it took is printed."""
import time

import numpy as np
import pytest

import long_vector_reference as lv
import minres_reference as mr
import test_gpu_csr as tc
import test_gpu_minres as mn

pytestmark = pytest.mark.gpu

DIAG5_SHIFTS = [0.0, 0.5, 4.0, -2.0]
_cache = {}
_spent = [0.0]


def _timed(key, make):
    """make(), once per session; prints what the reference cost and the module's total so far."""
    if key not in _cache:
        t0 = time.perf_counter()
        _cache[key] = make()
        dt = time.perf_counter() - t0
        _spent[0] += dt
        print("reference %r: made in %.2f s (this module so far: %.2f s)" % (key, dt, _spent[0]))
    return _cache[key]


def _reference(oracle, kind, n, shifts, max_iter, tol):
    return _timed((kind, n, tuple(shifts), max_iter, tol), lambda: mn._reference(oracle, kind, n, shifts, max_iter, tol))


def _same(a, b, rows_a, rows_b, what):
    """Rows rows_a of solve a = (X, res) equal rows rows_b of solve b: X bit for bit and every reported number."""
    (Xa, ra), (Xb, rb) = a, b
    ta, tb = mn._tuples(ra), mn._tuples(rb)
    for i, j in zip(rows_a, rows_b):
        assert np.array_equal(Xa[i], Xb[j]), (what, i, j, int(np.count_nonzero(Xa[i] != Xb[j])))
        assert ta[i] == tb[j], (what, i, j, ta[i], tb[j])


def _check_ends(X, res, ref, shifts, what):
    """A run that ends by a breakdown, by running out or without a launch against the reference: iterations and converged exactly,
    x within SHIFT_X_BOUND (exactly 0 where the reference's is), both residuals within RESIDUAL_BOUND (exactly 0 where the
    reference's is), x_norm within NORM_BOUND.  Returns the worst deviations."""
    worst = [0.0, 0.0]
    for j, sigma in enumerate(shifts):
        q = ref[j]
        assert (res[j]["iterations"], res[j]["converged"]) == (q["iterations"], q["converged"]), (what, sigma, res[j], q)
        nx = np.linalg.norm(q["x"])
        err = float(np.linalg.norm(X[j] - q["x"]) / nx) if nx > 0 else float(np.abs(X[j]).max())
        offs = [abs(res[j][k] - q[k]) / q[k] if q[k] > 0 else abs(res[j][k]) for k in ("residual_prev", "residual_last")]
        print("%s sigma=%g: (%d, %d), |dx|/|x| = %.2e, residual_prev off by %.2e, residual_last by %.2e" % (
            what, sigma, res[j]["iterations"], res[j]["converged"], err, offs[0], offs[1]))
        assert err <= (mn.SHIFT_X_BOUND if nx > 0 else 0.0), (what, sigma, err)
        assert max(offs) <= mn.RESIDUAL_BOUND and (q["residual_last"] > 0 or res[j]["residual_last"] == 0.0), (what, sigma, res[j], q)
        xn = float(np.linalg.norm(X[j]))
        assert abs(res[j]["x_norm"] - xn) <= mn.NORM_BOUND * xn, (what, sigma, res[j]["x_norm"], xn)
        assert res[j]["residual_last"] <= res[j]["residual_prev"], (what, sigma, res[j])
        worst = [max(worst[0], err), max(worst[1], *offs)]
    return worst


# ---- A1. the loop's ends: a breakdown found by the close kernel, max_iter = 4 and 0 -------------------------------------------------
@pytest.mark.parametrize("storage", ["dense", "csr"])
def test_loop_ends_on_diag5(gpu_pkg, oracle, storage):
    n, S = 600, DIAG5_SHIFTS
    A, b, _ = mn._problem(oracle, "diag5", n)
    d = np.diag(A)
    runs = {}
    with mn._solver(gpu_pkg, oracle, "diag5", n, storage) as s:
        if storage == "csr":
            assert s.gemv_plan()["R"] == 1, s.gemv_plan()
        s.tolerance(0.0)
        for max_iter in (n, 5, 4, 0):
            s.set_max_iter(max_iter)
            runs[max_iter] = s.solve_minres(S)
        s.set_source_term(np.zeros(n))
        zero = s.solve_minres(S)                    # max_iter = 0 and b = 0: no launch runs
        s.set_source_term(b)
        s.set_max_iter(5)
        again = s.solve_minres(S)
    for max_iter in (5, 4, 0):
        X, res = runs[max_iter]
        _check_ends(X, res, _reference(oracle, "diag5", n, S, max_iter, 0.0), S, "diag5 %s max_iter=%d" % (storage, max_iter))
    # max_iter = 5: the close kernel finds the breakdown the step kernel finds in launch 5 of the long run
    X, res = runs[5]
    assert [(r["iterations"], r["converged"]) for r in res] == [(4, 1), (4, 1), (4, 0), (4, 0)], res
    assert res[0]["residual_last"] == res[1]["residual_last"] == 0.0
    for j in (0, 1):
        assert np.abs(X[j] - 1.0 / (d + S[j])).max() <= 1e-13, (S[j], np.abs(X[j] - 1.0 / (d + S[j])).max())
    _same(runs[5], runs[n], range(4), range(4), "close kernel against step kernel")
    _same(again, runs[5], range(4), range(4), "after b = 0")
    # max_iter = 4: nothing breaks down
    assert [(r["iterations"], r["converged"]) for r in runs[4][1]] == [(4, 0)] * 4, runs[4][1]
    for r, want in zip(runs[4][1], (4.40, 3.55, 10.95, 10.95)):
        assert abs(r["residual_last"] - want) < 0.006, (r, want)
    # max_iter = 0
    nb = float(np.linalg.norm(b))
    X, res = runs[0]
    assert not X.any()
    for r in res:
        assert (r["iterations"], r["converged"], r["x_norm"], r["rel_residual"]) == (0, 0, 0.0, 1.0), r
        assert abs(r["residual_prev"] - nb) <= mn.RESIDUAL_BOUND * nb and r["residual_last"] == r["residual_prev"], (r, nb)
    X, res = zero
    _check_ends(X, res, mr.minres(A, np.zeros(n), S, 0, 0.0), S, "diag5 %s max_iter=0 b=0" % storage)
    assert not X.any()
    for r in res:
        assert tuple(r[k] for k in mn.KEYS[:5]) == (0, 1, 0.0, 0.0, 0.0), r


# ---- A2. convergence in the last column ---------------------------------------------------------------------------------------------
def test_convergence_in_the_last_column(gpu_pkg, oracle):
    n, tol = 257, 1e-10
    _, _, S8 = mn._problem(oracle, "lap2d", n)
    S = S8[:4] + S8[6:]                          # without the two interior shifts
    assert S[5] == -1e4

    def run(s, max_iter):
        s.set_max_iter(max_iter)
        return s.solve_minres(S)

    with mn._solver(gpu_pkg, oracle, "lap2d", n) as s:
        s.tolerance(tol)
        long_run = run(s, n)
        its = [r["iterations"] for r in long_run[1]]
        print("last column: iterations of the long run", its)
        assert all(r["converged"] == 1 for r in long_run[1]), long_run[1]
        big = int(np.argmax(its))
        assert its[5] < 10 and 64 < its[big] < n - 1, its      # 3 and 85 in the reference: under one poll, and over five
        cut = {(j, extra): run(s, its[j] + extra) for j in (5, big) for extra in (1, 0)}
    with mn._solver(gpu_pkg, oracle, "lap2d", n, check_every=1) as s:
        s.tolerance(tol)
        for (j, extra), out in cut.items():
            _same(run(s, its[j] + extra), out, range(len(S)), range(len(S)), ("check_every = 1", S[j], extra))
    for j in (5, big):
        m = its[j]
        # max_iter = m + 1: column m is closed by k_minres_close and freezes the shift there, converged
        at_end = [i for i in range(len(S)) if its[i] <= m]
        assert j in at_end
        _same(cut[j, 1], long_run, at_end, at_end, ("max_iter = m + 1", S[j]))
        for i in range(len(S)):
            if its[i] > m:
                r = cut[j, 1][1][i]
                assert (r["iterations"], r["converged"]) == (m + 1, 0) and r["residual_prev"] >= r["residual_last"] >= tol, (S[i], r)
        # max_iter = m: column m is never closed
        before = [i for i in range(len(S)) if its[i] < m]
        _same(cut[j, 0], long_run, before, before, ("max_iter = m", S[j]))
        for i in range(len(S)):
            if its[i] >= m:
                r = cut[j, 0][1][i]
                assert (r["iterations"], r["converged"]) == (m, 0) and r["residual_prev"] >= r["residual_last"] >= tol, (S[i], r)
        r = cut[j, 0][1][j]
        assert r["residual_last"] == long_run[1][j]["residual_prev"], (r, long_run[1][j])   # |phibar_m| in front of column m


# ---- A3. launch 0 and the non-finite rule -------------------------------------------------------------------------------------------
LAUNCH0 = [("hash0", 513, "dense"), ("lap2d", 1000, "csr")]


@pytest.mark.parametrize("kind,n,storage", LAUNCH0)
def test_zero_and_infinite_source_term(gpu_pkg, oracle, kind, n, storage):
    S, iters = [0.0, -2.0], 12
    _, b, _ = mn._problem(oracle, kind, n)
    binf = b.copy()
    binf[n // 2] = np.inf
    with mn._solver(gpu_pkg, oracle, kind, n, storage) as s:
        s.set_max_iter(iters)
        s.tolerance(1e-10)
        s.set_source_term(np.zeros(n))
        X0, res0 = s.solve_minres(S)
        s.set_source_term(binf)
        Xi, resi = s.solve_minres(S)
        s.set_source_term(b)
        s.tolerance(0.0)
        after = s.solve_minres(S)
    with mn._solver(gpu_pkg, oracle, kind, n, storage) as s:
        s.set_max_iter(iters)
        s.tolerance(0.0)
        fresh = s.solve_minres(S)
    assert not X0.any() and not Xi.any()
    for r in res0:
        assert tuple(r[k] for k in mn.KEYS[:5]) == (0, 1, 0.0, 0.0, 0.0), r
    for r in resi:
        assert (r["iterations"], r["converged"], r["x_norm"]) == (0, 0, 0.0), r
        assert not np.isfinite(r["residual_prev"]) and not np.isfinite(r["residual_last"]), r
        assert not (np.isfinite(r["rel_residual"]) and r["rel_residual"] < 1.0), r
    # nothing that is not finite outlives the solve: Ap, the partials, the side block
    assert np.isfinite(fresh[0]).all() and [r["iterations"] for r in fresh[1]] == [iters] * 2
    _same(after, fresh, range(2), range(2), "after b = 0 and an infinite b")


@pytest.mark.parametrize("kind,n,storage", LAUNCH0)
def test_huge_shifts_freeze_in_column_0(gpu_pkg, oracle, kind, n, storage):
    S, iters = [0.0, 1e200, -1e200, 1.0], 12
    A, b, _ = mn._problem(oracle, kind, n)
    with mn._solver(gpu_pkg, oracle, kind, n, storage) as s:
        s.set_max_iter(iters)
        s.tolerance(0.0)
        X, res = s.solve_minres(S)
        pair = s.solve_minres([0.0, 1.0])
    ref = _reference(oracle, kind, n, S, iters, 0.0)
    nb = float(np.linalg.norm(b))
    for j in (1, 2):
        assert (ref[j]["iterations"], ref[j]["converged"]) == (0, 0) and not ref[j]["x"].any()
        r = res[j]
        assert not X[j].any() and (r["iterations"], r["converged"], r["x_norm"], r["rel_residual"]) == (0, 0, 0.0, 1.0), r
        assert abs(r["residual_prev"] - nb) <= mn.RESIDUAL_BOUND * nb and r["residual_last"] == r["residual_prev"], (r, nb)
    _same((X, res), pair, (0, 3), (0, 1), "beside two frozen shifts")
    absA = np.abs(A)
    mn._check_against_reference(X[[0, 3]], [res[0], res[3]], [ref[0], ref[3]], lambda x: A @ x, lambda x: absA @ x, b, [0.0, 1.0], iters,
                                6 if kind == "lap2d" else n, "huge shifts %s n=%d %s" % (kind, n, storage))


# ---- A4. long vectors at every width, with freezing and a breakdown -----------------------------------------------------------------
def test_long_vectors_every_width_with_freezing(gpu_pkg):
    n, iters, tol, S = lv.N_LONG, 12, mr.LONG_TOL, mr.LONG_SHIFTS
    assert n > lv.N_STRIDED and len(S) == len(set(S)) == 16
    csr = tc.lap2d_csr(n)
    b = lv.normal_b(n)
    a, f = S.index(-3.7), S.index(-20.0)
    with gpu_pkg.CGSolver(gemv_variant=-1, matrix_format=gpu_pkg.MATRIX_CSR) as s:
        s.generate_lap2d_matrix(n)
        s.set_source_term(b)
        assert s.gemv_plan()["variant"] == 7, s.gemv_plan()
        s.set_max_iter(iters)
        s.tolerance(tol)
        wide = s.solve_minres(S)
        narrow = [s.solve_minres(sub) for sub in ([-3.7], [-3.7, -20.0], [1e3, -20.0, -3.7])]   # widths 1, 2, 4
    ref = _timed(("long lap2d", n), lambda: mr.minres(csr, b, S, iters, tol))
    its = [(q["iterations"], q["converged"]) for q in ref]
    print("long lap2d: (iterations, converged) of the reference", dict(zip(S, its)))
    assert [its[S.index(v)] for v in (100.0, -20.0, -1e4, 30.0, 1e3)] == [(5, 1), (9, 1), (2, 1), (7, 1), (3, 1)], its
    assert its[a] == (12, 0) and sum(c for _, c in its) == 8, its
    absdata = np.abs(csr[2])
    mn._check_against_reference(wide[0], wide[1], ref, lambda x: lv.matvec(csr[0], csr[1], csr[2], x),
                                lambda x: lv.matvec(csr[0], csr[1], absdata, x), b, S, None, 6, "long csr 16 wide n=%d" % n)
    _same(narrow[0], wide, [0], [a], "width 1")
    _same(narrow[1], wide, [0, 1], [a, f], "width 2")
    _same(narrow[2], wide, [0, 1, 2], [S.index(1e3), f, a], "width 4")


def test_long_vectors_breakdown(gpu_pkg):
    """diag(1, 2, 3, -4, -5 cycling) as CSR with one entry per row: the breakdown of test_breakdown_and_singular_shifts on the
    striding trip, found by the step kernel (max_iter = n) and by the close kernel (max_iter = 5)."""
    n, S = lv.N_LONG, DIAG5_SHIFTS
    d = np.array([1.0, 2.0, 3.0, -4.0, -5.0])[np.arange(n) % 5]
    csr = (np.arange(n + 1), np.arange(n), d)
    b = np.ones(n)
    with gpu_pkg.CGSolver(gemv_variant=-1, matrix_format=gpu_pkg.MATRIX_CSR) as s:
        s.set_matrix_csr(*csr, n)
        s.set_source_term(b)
        assert s.gemv_plan()["R"] == 1, s.gemv_plan()
        s.tolerance(0.0)
        s.set_max_iter(n)
        by_step = s.solve_minres(S)
        s.set_max_iter(5)
        by_close = s.solve_minres(S)
    ref = _timed(("long diag5", n), lambda: mr.minres(csr, b, S, n, 0.0))
    assert [(q["iterations"], q["converged"]) for q in ref] == [(4, 1), (4, 1), (4, 0), (4, 0)], ref
    for what, (X, res) in (("step", by_step), ("close", by_close)):
        _check_ends(X, res, ref, S, "long diag5 breakdown in the %s kernel" % what)
        for j in (0, 1):
            err = np.abs(X[j] - 1.0 / (d + S[j])).max()
            print("long diag5 %s sigma=%g: max |x - 1 / (d + sigma)| = %.2e" % (what, S[j], err))
            assert res[j]["residual_last"] == 0.0 and err <= 1e-13, (what, S[j], err)
    _same(by_close, by_step, range(4), range(4), "close kernel against step kernel")


# ---- A5. dense past 256 K1 partials and past 16 tiles -------------------------------------------------------------------------------
def _hash0_problem(oracle, n):
    """The hash0 problem of tests/test_gpu_minres.py with minres_reference.tile_shifts, so that no eigenvalue is computed: placed
    where _problem, _solver and _reference of that module look for it."""
    key = ("problem", "hash0", n)
    if key not in mn._cache:
        A, b = oracle.hash_rows(n, 0, n, mn.SEED, True, 0.0), np.cos(np.arange(n, dtype=np.float64))
        A.setflags(write=False)
        b.setflags(write=False)
        mn._cache[key] = (A, b, mr.tile_shifts(n))
    return mn._cache[key]


@pytest.mark.parametrize("n,trip,slot", [(1028, 0, 1), (2052, 0, 2), (4100, 1, 0)])
def test_dense_past_256_partials(gpu_pkg, oracle, n, trip, slot):
    """The last K1 partial, index ceil(n / 4) - 1, is alone in load slot `slot` of trip `trip` of fold_pap (thread 0)."""
    iters = 12
    A, b, S = _hash0_problem(oracle, n)
    assert S == mr.tile_shifts(n)
    nk1p = -(-n // 4)
    with mn._solver(gpu_pkg, oracle, "hash0", n, gemv_variant=-1) as s:
        plan = s.gemv_plan()
        assert plan["variant"] == 1 and plan["R"] == 4 and plan["split"] == 1 and plan["grid"] == nk1p, plan   # 4 rows per workgroup
        s.set_max_iter(iters)
        s.tolerance(0.0)
        X, res = s.solve_minres(S)
    last = nk1p - 1
    print("n=%d: %d K1 partials (the last in trip %d, slot %d of fold_pap), %d row tiles, %d rows in the last" % (
        n, nk1p, last // 1024, last % 1024 // 256, -(-n // 256), n - (n - 1) // 256 * 256))
    assert last % 256 == 0 and (last // 1024, last % 1024 // 256) == (trip, slot)
    absA = np.abs(A)
    mn._check_against_reference(X, res, _reference(oracle, "hash0", n, S, iters, 0.0), lambda x: A @ x, lambda x: absA @ x, b, S, iters, n,
                                "past 256 partials n=%d" % n)


# ---- A6. ldx > n, and a second problem in one context ---------------------------------------------------------------------------------
def test_ldx_beyond_n(gpu_pkg, oracle):
    cgx = gpu_pkg.cgx
    n, pad = 257, 5
    sig = np.array([0.0, -1.0, 50.0])
    with mn._solver(gpu_pkg, oracle, "lap2d", n) as s:
        s.set_max_iter(12)
        s.tolerance(0.0)
        X, res = s.solve_minres(sig)
        Xw = np.full((3, n + pad), 7.0)
        out = (cgx.Result * 3)()
        assert cgx.lib().cgx_solve_minres(s._h, 3, cgx._dp(sig), cgx._dp(Xw), n + pad, out) == 0
    assert np.isfinite(X).all() and X.any(axis=1).all()
    assert (Xw[:, n:] == 7.0).all()
    _same((Xw[:, :n], [out[j].as_dict() for j in range(3)]), (X, res), range(3), range(3), "ldx = n + 5")


def test_second_problem_in_one_context(gpu_pkg, oracle):
    """n = 1000, 257, 1000 in one context: free_problem frees the side block and ensure_side_block makes it anew, smaller, then
    larger.  Each solve has the bits of a context that never held another problem."""
    S, sizes = [0.0, 1.0, -1.0, 100.0, -1e4], (1000, 257, 1000)

    def solve(s, n):
        s.generate_lap2d_matrix(n)
        s.init_source_term(1.0 / n)
        s.set_max_iter(12)
        s.tolerance(1e-8)
        return s.solve_minres(S)

    with gpu_pkg.CGSolver(gemv_variant=-1) as s:
        outs = [solve(s, n) for n in sizes]
    fresh = {}
    for n in set(sizes):
        with gpu_pkg.CGSolver(gemv_variant=-1) as s:
            fresh[n] = solve(s, n)
    for n, out in zip(sizes, outs):
        X, res = out
        assert X.shape == (len(S), n) and np.isfinite(X).all() and X.any(axis=1).all()
        assert res[4]["converged"] == 1 and res[0]["converged"] == 0, res
        _same(out, fresh[n], range(len(S)), range(len(S)), "problem of size %d" % n)
