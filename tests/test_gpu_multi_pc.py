"""cgx_solve_multi_pc (csrc/cgx_multi_pc.hip) on the MI355X: several right-hand sides with the context's
preconditioner, every column its own PCG.

1. fixed iterations with the pivoted-Cholesky factor against numpy PCG in fp64 and longdouble with the device's own L and delta;
2. converged columns: exact iteration counts where the stop is not a matter of rounding;
3. point Jacobi on S lap2d S with a diagonal that differs from row to row;
4. every column against a single solve on the same context, which the multi call must leave as it was;
5. z = M^-1 r of the multi kernels against the single path's, bit for bit;
6. independence: permuted columns, other companions, check_every;
7. columns that break many iterations apart, frozen columns;
8. no preconditioner: the bits of solve_multi;
9. the refusals (solve_multi's own refusal of a preconditioner included);
10. the walk over every runtime call of a solve with an injected failure (host side: nothing faults on the device).
Every reference number is computed here; none is hard-coded."""
import numpy as np
import pytest

import multi_pc_reference as mref
import pivchol_reference as ref

pytestmark = pytest.mark.gpu

BAD_ARG, ERR_HIP, UNSUPPORTED = 1, 3, 7   # cgx_status (include/cgx.h)
ELL, SIGMA2 = 0.2, 1e-2
SHAPES = [(1024, 1), (1024, 5), (1024, 64), (1024, 100), (1024, 256), (1000, 64), (1101, 64)]   # the odd sizes: a ragged last tile
KEYS = ("iterations", "converged", "residual_prev", "residual_last", "x_norm", "rel_residual")
_CACHE = {}


# ---- problems ------------------------------------------------------------------------------------------------------------------
def _kernel_problem(n):
    """(A, b, the 16 right-hand sides, the 16 guesses) of the kernel matrix; a k-column test takes the first k."""
    if ("kp", n) not in _CACHE:
        A, b = ref.kernel_matrix(n, ELL, SIGMA2)
        _CACHE[("kp", n)] = (A, b, mref.rhs_block(A, b, 16), mref.x0_block(n, 16))
    return _CACHE[("kp", n)]


def _kernel_solver(gpu_pkg, n, rank, **kw):
    A, b, _, _ = _kernel_problem(n)
    s = gpu_pkg.CGSolver(gemv_variant=kw.pop("gemv_variant", -1), **kw)
    s.set_matrix_dense(A)
    s.set_source_term(b)
    s.set_max_iter(3000)
    s.tolerance(1e-6 * float(np.linalg.norm(b)))
    if rank:
        s.set_preconditioner("pivchol", rank=rank)
    return s


def _jacobi_problem(oracle, n=1024):
    if ("jp", n) not in _CACHE:
        A = mref.scaled_lap2d(oracle.generate_lap2d(n))
        _CACHE[("jp", n)] = (A, mref.rhs_block(A, oracle.init_source_term(n), 16), mref.x0_block(n, 16))
    return _CACHE[("jp", n)]


def _jacobi_solver(gpu_pkg, oracle, n=1024, **kw):
    A, B, _ = _jacobi_problem(oracle, n)
    s = gpu_pkg.CGSolver(gemv_variant=-1, **kw)
    s.set_matrix_dense(A)
    s.set_source_term(B[0])
    s.set_preconditioner("jacobi")
    return s


def _references(key, A, B, X0, applies, tol, iters):
    """fp64 and longdouble PCG of every column, once per key."""
    if key not in _CACHE:
        _CACHE[key] = (mref.pcg_block(A, B, X0, applies[0], tol, iters, np.float64),
                       mref.pcg_block(A, B, X0, applies[1], tol, iters, ref.LD))
    return _CACHE[key]


def _check_x(x, r64, rld, what):
    """|x - x_ld| / |x_ld| <= max(100 dist, 1e-12), dist = the distance of numpy's fp64 run from the longdouble run
    (the margin of test_gpu_pivchol._check_solve)."""
    nrm = np.linalg.norm(rld["x"])
    dist = float(np.linalg.norm(r64["x"] - rld["x"]) / nrm)
    got = float(np.linalg.norm(x - rld["x"]) / nrm)
    print("%s: |x - x_ld|/|x_ld| = %.3e, numpy fp64 %.3e, bar %.3e" % (what, got, dist, max(100 * dist, 1e-12)))
    assert got <= max(100 * dist, 1e-12), (what, got, dist)


def _bits(a, b, what=None):
    (Xa, ra), (Xb, rb) = a, b
    assert np.array_equal(Xa, Xb), what
    for j in range(len(ra)):
        for key in KEYS:
            assert ra[j][key] == rb[j][key], (what, j, key, ra[j][key], rb[j][key])


# ---- 1. fixed iterations, pivoted Cholesky -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,rank", SHAPES)
def test_fixed_iterations_pivchol(gpu_pkg, n, rank):
    iters = 12
    A, _, B, X0 = _kernel_problem(n)
    out = {}
    with _kernel_solver(gpu_pkg, n, rank) as s:
        s.set_max_iter(iters)
        s.tolerance(0.0)
        for k in (1, 2, 3, 5, 8, 9, 16):
            out[k] = s.solve_multi_pc(B[:k], X0[:k])
        _, L, delta = s._probe_precond_lowrank()
    r64, rld = _references(("fix", n, rank), A, B, X0, (ref.Woodbury(L, delta, np.float64).apply, ref.Woodbury(L, delta, ref.LD).apply),
                           0.0, iters)
    for k, (X, res) in out.items():
        for j in range(k):
            assert res[j]["iterations"] == iters == rld[j]["iterations"] and res[j]["converged"] == 0, (k, j, res[j])
            _check_x(X[j], r64[j], rld[j], "n=%d rank=%d k=%d column %d" % (n, rank, k, j))
            assert res[j]["gemv_bytes"] == 8.0 * (n * n + 2.0 * k * n)


# ---- 2. converged, pivoted Cholesky ----------------------------------------------------------------------------------------------
def test_converged_pivchol(gpu_pkg):
    n, rank, k = 1024, 64, 8
    A, b, B16, _ = _kernel_problem(n)
    B, X0 = B16[:k], np.zeros((k, n))
    tol = 1e-6 * float(np.linalg.norm(b))
    with _kernel_solver(gpu_pkg, n, rank) as s:
        X, res = s.solve_multi_pc(B)
        _, L, delta = s._probe_precond_lowrank()
    r64, rld = _references(("conv", n, rank), A, B, X0, (ref.Woodbury(L, delta, np.float64).apply, ref.Woodbury(L, delta, ref.LD).apply),
                           tol, 400)
    clear = 0
    for j in range(k):
        kj = rld[j]["iterations"]
        # the stop is not a matter of rounding: both references stop at kj, clearly below tol there and clearly above it one step
        # earlier (the rule of test_gpu_pivchol._references)
        is_clear = r64[j]["iterations"] == kj and all(r["hist"][kj + 1] <= 0.95 * tol and r["hist"][kj] >= 1.05 * tol for r in (r64[j], rld[j]))
        clear += is_clear
        print("column %d: device %d, fp64 %d, longdouble %d (stop at %.3f tol, %.3f tol one step earlier)%s" % (
            j, res[j]["iterations"], r64[j]["iterations"], kj, rld[j]["hist"][kj + 1] / tol, rld[j]["hist"][kj] / tol, " clear" if is_clear else ""))
        assert res[j]["converged"] == 1 and rld[j]["converged"] == 1, (j, res[j])
        assert res[j]["rel_residual"] <= 10 * tol / float(np.linalg.norm(B[j])), (j, res[j])
        if is_clear:
            assert res[j]["iterations"] == kj, (j, res[j], kj)
        else:
            assert abs(res[j]["iterations"] - kj) <= 1, (j, res[j], kj)
        _check_x(X[j], r64[j], rld[j], "column %d" % j)
    assert clear >= 5, clear


# ---- 3. Jacobi -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [3, 16])
def test_jacobi(gpu_pkg, oracle, k):
    n, iters = 1024, 20
    A, B16, X16 = _jacobi_problem(oracle, n)
    B, X0 = B16[:k], X16[:k]
    applies = (mref.jacobi_apply(A, np.float64), mref.jacobi_apply(A, ref.LD))
    with _jacobi_solver(gpu_pkg, oracle, n) as s:
        s.set_max_iter(iters)
        s.tolerance(0.0)
        Xf, resf = s.solve_multi_pc(B, X0)
        s.set_max_iter(n)
        s.tolerance(1e-10)
        Xc, resc = s.solve_multi_pc(B, X0)
    op = mref.CsrOp(A)
    r64, rld = _references(("jfix", n), op, B16, X16, applies, 0.0, iters)
    for j in range(k):
        assert resf[j]["iterations"] == iters and resf[j]["converged"] == 0, (j, resf[j])
        _check_x(Xf[j], r64[j], rld[j], "Jacobi k=%d column %d" % (k, j))
    _, cld = _references(("jconv", n), op, B16, X16, applies, 1e-10, n)
    for j in range(k):
        ro = cld[j]
        print("Jacobi converged column %d: device %d iterations, longdouble %d; rel_residual %.3e / %.3e" % (
            j, resc[j]["iterations"], ro["iterations"], resc[j]["rel_residual"], ro["rel_residual"]))
        assert resc[j]["converged"] == 1 and ro["converged"] == 1, (j, resc[j])
        assert abs(resc[j]["iterations"] - ro["iterations"]) <= 0.15 * ro["iterations"] + 1, (j, resc[j], ro["iterations"])
        assert resc[j]["rel_residual"] <= max(1e-11, 4.0 * ro["rel_residual"]), (j, resc[j], ro["rel_residual"])


# ---- 4. against single solves on the same context -----------------------------------------------------------------------------------
def _single(s, b, iters):
    s.set_source_term(b)
    x = np.zeros(len(b))
    return x, s.solve(x)


def _against_single(make, B, expect_variant=None):
    """make(): a fresh context with matrix, preconditioner and tol = 0.  Multi against single at 3 and 12 iterations; the plan
    stays; a single solve behind the multi call has the bits of a fresh context's, and so has a multi call behind a single one."""
    k, n = B.shape
    with make() as s:
        plan = s.gemv_plan()
        for iters in (3, 12):
            s.set_max_iter(iters)
            X, res = s.solve_multi_pc(B)
            assert s.gemv_plan() == plan
            for j in range(k):
                x, r = _single(s, B[j], iters)
                assert res[j]["iterations"] == r["iterations"] == iters, (j, res[j], r)
                d = np.linalg.norm(X[j] - x) / np.linalg.norm(x)
                assert d <= 1e-12, (iters, j, d)
            assert s.gemv_plan() == plan
        s.set_max_iter(12)
        first_multi = s.solve_multi_pc(B)
        after = _single(s, B[0], 12)
        s.set_preconditioner(None)
        if expect_variant is not None:
            assert s.gemv_plan()["variant"] == expect_variant, s.gemv_plan()
    with make() as s:
        s.set_max_iter(12)
        fresh = _single(s, B[0], 12)          # (makes the inverse diagonal / the factor)
        second_multi = s.solve_multi_pc(B)    # ... which the multi call now takes over
    assert np.array_equal(after[0], fresh[0])
    for key in KEYS:
        assert after[1][key] == fresh[1][key], key
    _bits(first_multi, second_multi, "multi first / single first")


@pytest.mark.parametrize("n", [2048, 4097, 10000])
def test_jacobi_against_single(gpu_pkg, monkeypatch, n):
    monkeypatch.delenv("CGX_RESIDENT", raising=False)   # the library's own choice: a persistent kernel up to n = 16384
    B = np.random.default_rng(n).standard_normal((3, n))
    seen = {}

    def make():
        s = gpu_pkg.CGSolver(gemv_variant=0)
        s.generate_lap2d_matrix(n)
        seen["plain"] = s.gemv_plan()
        s.set_preconditioner("jacobi")
        s.tolerance(0.0)
        return s

    _against_single(make, B, expect_variant=4 if n == 2048 else None)
    with gpu_pkg.CGSolver(gemv_variant=0) as s:           # the context's plan is a persistent kernel, which the Jacobi kind parks
        s.generate_lap2d_matrix(n)
        plain = s.gemv_plan()
        s.set_preconditioner("jacobi")
        assert s.gemv_plan() != plain, (plain, s.gemv_plan())
        s.set_preconditioner(None)
        assert s.gemv_plan() == plain == seen["plain"]


def test_pivchol_against_single(gpu_pkg):
    n = 1024
    _, _, B16, _ = _kernel_problem(n)

    def make():
        s = _kernel_solver(gpu_pkg, n, 32)
        s.tolerance(0.0)
        return s

    _against_single(make, B16[:3])
    with make() as s:                                     # the factor of the multi call is the single path's
        assert s.preconditioner_shift() == (0.0, 0.0)
        s.set_max_iter(2)
        s.solve_multi_pc(B16[:2])
        delta = s.preconditioner_shift()[1]
        assert delta > 0.0
        _, L, d2 = s._probe_precond_lowrank()
        assert d2 == delta and L.shape == (n, 32)


# ---- 5. the apply ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,rank", SHAPES)
def test_apply_matches_the_single_path(gpu_pkg, n, rank):
    _, _, B16, _ = _kernel_problem(n)
    R = np.array(B16)
    R[5] = 0.0
    R[5, 7] = 1.0
    with _kernel_solver(gpu_pkg, n, rank) as s:
        s.set_max_iter(1)
        s.tolerance(0.0)
        s.solve_multi_pc(R[:3])                           # the multi call makes the factor ...
        single = np.array([s._probe_precond_apply(R[j]) for j in range(16)])   # ... the single path's kernels use it
        for k in (1, 2, 3, 5, 8, 9, 16):
            Z = s._probe_multi_pc_apply(R[:k])
            assert np.all(np.isfinite(Z)) and np.linalg.norm(Z) > 0
            assert np.array_equal(Z.view(np.uint64), single[:k].view(np.uint64)), (k, float(np.abs(Z - single[:k]).max()))


def test_apply_jacobi(gpu_pkg, oracle):
    n = 1024
    A, B16, _ = _jacobi_problem(oracle, n)
    with _jacobi_solver(gpu_pkg, oracle, n) as s:
        for k in (3, 16):
            Z = s._probe_multi_pc_apply(B16[:k])
            assert np.array_equal(Z, (1.0 / np.diag(A))[None, :] * B16[:k])


# ---- 6. independence ------------------------------------------------------------------------------------------------------------------
def _independence(make, B, X0):
    k = B.shape[0]
    perm = np.random.default_rng(1).permutation(k)
    with make(check_every=1) as s:
        X, res = s.solve_multi_pc(B, X0)
        Xp, resp = s.solve_multi_pc(B[perm], X0[perm])
        B2 = B.copy()
        B2[1:] = B2[1:][::-1] * 3.0                       # column 0 among other companions, same k
        X2, res2 = s.solve_multi_pc(B2, X0)
    assert all(r["converged"] == 1 for r in res) and len(set(r["iterations"] for r in res)) > 1, res
    _bits((Xp, resp), (X[perm], [res[p] for p in perm]), "permuted")
    _bits((X2[:1], res2[:1]), (X[:1], res[:1]), "companions")
    for every in (7, 16):
        with make(check_every=every) as s:
            _bits(s.solve_multi_pc(B, X0), (X, res), "check_every %d" % every)


def test_independence_pivchol(gpu_pkg):
    n = 1101
    _, _, B16, X16 = _kernel_problem(n)
    _independence(lambda **kw: _kernel_solver(gpu_pkg, n, 64, **kw), B16[:8], X16[:8])


def test_independence_jacobi(gpu_pkg, oracle):
    _, B16, X16 = _jacobi_problem(oracle)

    def make(**kw):
        s = _jacobi_solver(gpu_pkg, oracle, **kw)
        s.set_max_iter(1024)
        s.tolerance(1e-8)
        return s

    _independence(make, B16[:8], X16[:8])


# ---- 7. columns that break apart ------------------------------------------------------------------------------------------------------
def _break_apart(make, A, b):
    n = len(b)
    x_known = np.sin(np.arange(n) * 0.01)
    B = np.array([b, 1e-3 * b, 1e3 * b, A @ x_known])
    X0 = np.zeros((4, n))
    X0[3] = x_known                                       # r0 = b - A x0 is rounding only: the column breaks at iteration 0
    with make() as s:
        X, res = s.solve_multi_pc(B, X0)
        its = [r["iterations"] for r in res]
        print("breaks at", its)
        assert all(r["converged"] == 1 for r in res), res
        assert its[3] == 0 and its[1] < its[0] < its[2] and its[2] - its[1] >= 6, its
        for j in range(4):                                # the column without its companions, stopped where it broke
            s.set_max_iter(its[j] + 1)
            Xa, ra = s.solve_multi_pc(np.tile(B[j], (4, 1)), np.tile(X0[j], (4, 1)))
            assert ra[0]["iterations"] == its[j] and ra[0]["converged"] == 1, (j, ra[0])
            assert np.array_equal(Xa[0], X[j]), j
            for key in KEYS:
                assert ra[0][key] == res[j][key], (j, key)


def test_columns_break_apart_pivchol(gpu_pkg):
    n = 1024
    A, b, _, _ = _kernel_problem(n)
    _break_apart(lambda: _kernel_solver(gpu_pkg, n, 16), A, b)


def test_columns_break_apart_jacobi(gpu_pkg, oracle):
    A, B16, _ = _jacobi_problem(oracle)

    def make():
        s = _jacobi_solver(gpu_pkg, oracle)
        s.set_max_iter(1024)
        s.tolerance(1e-6 * float(np.linalg.norm(B16[0])))
        return s

    _break_apart(make, A, B16[0])


# ---- 8. no preconditioner --------------------------------------------------------------------------------------------------------------
def test_no_preconditioner_is_solve_multi(gpu_pkg):
    n = 1101
    _, _, B16, X16 = _kernel_problem(n)
    with _kernel_solver(gpu_pkg, n, 0) as s:
        s.set_max_iter(60)
        for k in (3, 16):
            X, res = s.solve_multi(B16[:k], X16[:k])
            Xp, resp = s.solve_multi_pc(B16[:k], X16[:k])
            assert np.array_equal(X.view(np.uint64), Xp.view(np.uint64))
            for j in range(k):
                for key in res[j]:
                    if not key.startswith("seconds_"):
                        a, b = res[j][key], resp[j][key]
                        assert a == b or (a != a and b != b), (k, j, key, a, b)


# ---- 9. refusals -------------------------------------------------------------------------------------------------------------------------
def _refused(gpu_pkg, s, B, status):
    with pytest.raises(gpu_pkg.CgxError) as e:
        s.solve_multi_pc(B)
    assert e.value.status == status, e.value
    return str(e.value)


def test_refusals(gpu_pkg):
    cgx = gpu_pkg.cgx
    n = 1024
    B = np.ones((2, n))
    with gpu_pkg.CGSolver(gemv_variant=-1) as s:
        s.generate_lap2d_matrix(n)
        s.set_preconditioner("jacobi", block=8)
        assert "block" in _refused(gpu_pkg, s, B, UNSUPPORTED)
        s.set_preconditioner("jacobi", block=1)
        X, res = s.solve_multi_pc(B)                      # point Jacobi runs on the same context
        assert all(r["converged"] for r in res)
        for kind in ("jacobi", "pivchol"):                # the old contract stands
            s.set_preconditioner(kind)
            with pytest.raises(cgx.CgxError) as e:
                s.solve_multi(B)
            assert e.value.status == UNSUPPORTED
    for kw in ({"comm_mode": cgx.COMM_LOOPBACK, "nranks": 2}, {"matrix_format": cgx.MATRIX_BANDED}, {"matrix_format": cgx.MATRIX_CSR}):
        for kind in (None, "jacobi"):
            with gpu_pkg.CGSolver(gemv_variant=-1, **kw) as s:
                s.generate_lap2d_matrix(n)
                s.set_preconditioner(kind)
                msg = _refused(gpu_pkg, s, B, UNSUPPORTED)
                with pytest.raises(cgx.CgxError) as e:    # ... in the words of cgx_solve_multi
                    s.set_preconditioner(None)
                    s.solve_multi(B)
                assert e.value.status == UNSUPPORTED and str(e.value).replace("cgx_solve_multi", "cgx_solve_multi_pc") == msg
    for kind in ("jacobi", "pivchol"):
        with gpu_pkg.CGSolver(gemv_variant=40000) as s:
            s.generate_lap2d_matrix(n)
            s.init_source_term(1.0 / n)
            s.set_preconditioner(kind)
            msg = _refused(gpu_pkg, s, B, UNSUPPORTED)
            with pytest.raises(cgx.CgxError) as e:        # the single solve's status and message
                s.solve(np.zeros(n))
            assert e.value.status == UNSUPPORTED and str(e.value) == msg
    with gpu_pkg.CGSolver(gemv_variant=-1) as s:
        for bad in (np.ones((0, n)), np.ones((17, n))):
            s.generate_lap2d_matrix(n)
            s.set_preconditioner("jacobi")
            _refused(gpu_pkg, s, bad, BAD_ARG)
    with gpu_pkg.CGSolver(gemv_variant=-1) as s:          # rank > n
        s.generate_lap2d_matrix(100)
        s.set_preconditioner("pivchol", rank=101)
        _refused(gpu_pkg, s, np.ones((2, 100)), BAD_ARG)


def test_a_matrix_that_is_not_positive_definite(gpu_pkg):
    n = 1024
    A, b, B16, _ = _kernel_problem(n)
    bad = np.array(A)
    bad[321, 321] = -1.0e6
    with gpu_pkg.CGSolver(gemv_variant=-1) as s:
        s.set_matrix_dense(bad)
        s.set_source_term(b)
        for kind in ("pivchol", "jacobi"):
            s.set_preconditioner(kind, rank=16) if kind == "pivchol" else s.set_preconditioner(kind)
            msg = _refused(gpu_pkg, s, B16[:3], BAD_ARG)
            assert "row 321" in msg, msg
        s.set_matrix_dense(A)                             # the context stays usable
        s.set_source_term(b)
        s.set_max_iter(3000)
        s.tolerance(1e-6 * float(np.linalg.norm(b)))
        s.set_preconditioner("pivchol", rank=16)
        got = s.solve_multi_pc(B16[:3])
    with _kernel_solver(gpu_pkg, n, 16) as s:
        _bits(s.solve_multi_pc(B16[:3]), got, "after a refused matrix")


# ---- 10. fault walk ----------------------------------------------------------------------------------------------------------------------
def test_fault_walk(gpu_pkg):
    import torch
    n, k, rank = 1024, 3, 8
    _, _, B16, X16 = _kernel_problem(n)
    B, X0 = B16[:k], X16[:k]
    with _kernel_solver(gpu_pkg, n, rank) as s:
        s.set_max_iter(40)
        ref_run = s.solve_multi_pc(B, X0)
        free0 = torch.cuda.mem_get_info()[0]

        def walk(before=None):
            calls = 0
            while True:
                if before:
                    before()
                s._set_fault_after(calls)
                try:
                    got = s.solve_multi_pc(B, X0)
                except gpu_pkg.CgxError as e:
                    assert e.status == ERR_HIP, (calls, e)
                    assert torch.cuda.mem_get_info()[0] == free0, calls
                    calls += 1
                    assert calls < 600
                    continue
                s._set_fault_after(-1)
                return calls, got

        calls, got = walk()                               # the factor stands: set-up, loop, polls, the end
        assert calls > 10, calls
        _bits(got, ref_run, "behind the walk")

        def stale():                                      # the factor goes stale, so every attempt makes it again
            s.set_preconditioner("pivchol", rank=rank + 1)
            s.set_preconditioner("pivchol", rank=rank)

        stale()
        s.solve_multi_pc(B, X0)
        free0 = torch.cuda.mem_get_info()[0]              # (the factor was allocated anew)
        calls2, got = walk(before=stale)
        assert calls2 > calls + rank, (calls, calls2)
        _bits(got, ref_run, "behind the walk over the set-up")
        _bits(s.solve_multi_pc(B, X0), ref_run, "once more")
        assert torch.cuda.mem_get_info()[0] == free0
