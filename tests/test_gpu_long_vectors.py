"""Block Jacobi and multi-shift CG on vectors of more than 262144 = 256 * kMaxVectorGrid rows (DESIGN.md sections 13 and 14).

Above that size the update kernels stride over the rows and K1's head folds more than 256 partials; each of the two features has
a long-vector form of its own that no smaller problem reaches.  Everything here runs on CSR storage at
n = N_LONG = 262144 + 5 * 256 + 77 = 263501 (tests/long_vector_reference.py): 1030 tiles on 1024 workgroups, so workgroups 0 - 5
take a second trip and the others none; the last tile holds 77 rows; the last block is truncated for every block size; n / 3
cuts blocks and tiles at shard boundaries.  The generator's matrix has the same tridiagonal Toeplitz block (4, -1) in every
tile, which hides a block inverse fetched for the wrong tile, so the block-Jacobi tests scale it row by row (A = S L S) or use a
block-diagonal matrix with a different block everywhere.  References: tests/long_vector_reference.py in longdouble, pinned on
the CPU by tests/test_long_vector_reference.py.

Which branch each test reaches:

a. test_block_jacobi_against_longdouble      k_update_xr_strided_bj<4 / 32 / 256> (the early-only chain, the chain past kBjEarly,
                                             the in-place inversion size), the second trip of k_init_residual_bj, the stride loop
                                             of k_csr_bj_col_slice, head_finish_pc's second loop (1024 partials per set); on 3
                                             loopback shards `own` differs from trip to trip and W is gathered slice by slice
b. test_block_jacobi_scaled_rows_give_the_unscaled_bits   the same kernels, bit for bit: a W row of another tile, a wrong block
                                             start inside a second-trip tile or a stale rl tile breaks it
c. test_block_jacobi_exact_on_a_block_diagonal_matrix     every block of W is read once, each one different: a wrong block in a
                                             second-trip tile alone leaves a residual
d. test_block_inverses_of_the_second_trip    W itself for every row from 262144 on (k_csr_bj_col_slice's second trip,
                                             k_bj_invert on the blocks past 262144 and on the truncated one)
e. test_zero_shift_is_the_plain_solve        fold_pap_strided in k_shift_update against k_update_xr_strided, rr_finish's loop over the
                                             partials from 256 on against head_finish's, pap_strided set by the host
f. test_every_shift_against_longdouble       k_shift_update<8>'s second loop (it reads P and X again), k_column_norms<true> and the
                                             |zeta| sqrt(r.r) stores: every reported number against a value computed outside
g. test_widths_and_companions                k_shift_update<1>, <8> and <16> in the second loop, masked shifts
h. test_a_frozen_shift_stays_frozen_in_the_second_trip   the skip on s_flag in the second loop, rows below and from 262144 on
                                             compared separately

Every test asserts n > 262144 and the plan it runs (the CSR variant and lane count from gemv_plan(), the number of shards, the
block size), and prints what it measured beside its bar.  Measured on an MI355X: a. 3.7e-16 ... 4.4e-16 against 1e-10; b. every
case the same bits; c. 2.6e-16 (block 8) and 5.0e-16 (block 32) against 1e-12, point Jacobi 0.45 / 0.49; f. x at most 8.9e-16
against 1e-12, the residuals at most 2.7e-15 against 1e-9, x_norm at most 1.8e-16; h. both row ranges at most 1.4e-16, the
stops at 7 and 3 as the reference's."""
import functools

import numpy as np
import pytest

import block_jacobi_reference as ref
import long_vector_reference as lv
import test_gpu_csr as tc
import test_gpu_shifted as ts
from test_gpu_jacobi_scaled import N_STRIDED, _check_rel_residual, _csr_products, _csr_rows, _shards

pytestmark = pytest.mark.gpu

N = lv.N_LONG
LD = np.longdouble
EPS = 2.0 ** -52
REL_BOUND = 1e-10          # tests/test_gpu_block_jacobi.py
SHIFT_X_BOUND = 1e-12      # tests/test_gpu_shifted.py test_fixed_iterations_against_oracle
RESIDUAL_BOUND = 1e-9      # tests/test_gpu_parity.py test_full_size_properties: reported residuals
NORM_BOUND = 1e-12
S7 = ts.S7


# ---- problems and references, made once ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _lap():
    """(indptr, indices, data, rows) of the generator's matrix at N, read-only."""
    assert N > N_STRIDED == lv.N_STRIDED and N == 263501
    indptr, indices, data = tc.lap2d_csr(N)
    out = (indptr, indices, data, _csr_rows(indptr))
    assert len(indptr) == N + 1 and np.all(np.diff(indptr) <= 5)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _vectors():
    s, b = lv.spread_scale(N), lv.normal_b(N)
    s.setflags(write=False)
    b.setflags(write=False)
    return s, b


@functools.lru_cache(maxsize=None)
def _sls():
    """S L S with s spread over [1, 100] and its right-hand side S b~."""
    indptr, indices, data, rows = _lap()
    s, bt = _vectors()
    scaled = s[rows] * data * s[indices]
    bs = s * bt
    scaled.setflags(write=False)
    bs.setflags(write=False)
    return scaled, bs


@functools.lru_cache(maxsize=None)
def _bj_reference(block):
    s, _ = _vectors()
    return lv.pcg_scaled_lap2d(N, s, _sls()[1], block, 12, LD)


@functools.lru_cache(maxsize=None)
def _shift_reference(sigma, iters, tol, keep=()):
    indptr, indices, data, _ = _lap()
    return lv.cg_shifted((indptr, indices, data), _vectors()[1], sigma, iters, tol, LD, keep)


def _pow2_scale(n, seed):
    """tests/test_gpu_block_jacobi.py section 6: every exponent of [-3, 3], permuted."""
    e = np.random.default_rng(seed).permutation(np.arange(n) % 7 - 3)
    assert e.min() == -3 and e.max() == 3
    return np.ldexp(1.0, e)


def _rel(x, want):
    return float(np.linalg.norm(x - want) / np.linalg.norm(want))


# ---- block Jacobi ---------------------------------------------------------------------------------------------------------------
def _bj_context(pkg, p, csr, block):
    """A CSR context of p shards with block Jacobi set, its plan asserted: every shard runs the CSR K1 (variant 7), and n is in
    the range where launch_update_xr takes k_update_xr_strided_bj (update_xr_grid(n) * 256 < n)."""
    c = tc.solver(pkg, p, gemv_variant=0)
    try:
        c.set_matrix_csr(*csr)
        c.set_preconditioner("jacobi", block=block)
        assert c.n() == N > N_STRIDED
        assert _shards(c) == p and all(c.gemv_plan(q)["variant"] == 7 for q in range(p)), [c.gemv_plan(q) for q in range(p)]
        assert c.preconditioner == "jacobi" and c.preconditioner_block() == block
        assert sum(c.matrix_nnz(q) for q in range(p)) == len(csr[2])
    except BaseException:
        c.close()
        raise
    return c


def _run(c, b, iters, tol=0.0):
    c.set_max_iter(iters)
    c.tolerance(tol)
    c.set_source_term(b)
    x = np.zeros(len(b))
    return x, c.solve(x)


@pytest.mark.parametrize("p", [1, 3])
@pytest.mark.parametrize("block", [4, 32, 256])
def test_block_jacobi_against_longdouble(gpu_pkg, block, p):
    indptr, indices, _, rows = _lap()
    scaled, bs = _sls()
    want = _bj_reference(block)
    with _bj_context(gpu_pkg, p, (indptr, indices, scaled), block) as c:
        x, res = _run(c, bs, 12)
    err = _rel(x, want["x"])
    xn = float(np.linalg.norm(x))
    print("longdouble block %d p=%d: |x - x_ref| / |x_ref| = %.3e (bar %.0e), x_norm off by %.3e" % (
        block, p, err, REL_BOUND, abs(res["x_norm"] - xn) / xn))
    assert res["iterations"] == want["iterations"] == 12 and res["converged"] == 0, res
    assert err <= REL_BOUND, (block, p, err)
    ax, aax = _csr_products(rows, indices, scaled, x, N)
    _check_rel_residual(res, ax, aax, bs, 5, (block, p))
    assert abs(res["x_norm"] - xn) <= NORM_BOUND * xn, (res["x_norm"], xn)


@pytest.mark.parametrize("p", [1, 3])
@pytest.mark.parametrize("block", [4, 32, 256])
def test_block_jacobi_scaled_rows_give_the_unscaled_bits(gpu_pkg, block, p):
    """s * x(S L S, S b) == x(L, b) on all n entries for s_i = 2**e_i, e_i in [-3, 3] permuted (tests/test_gpu_block_jacobi.py
    section 6 has the argument), 30 iterations."""
    iters = 30
    indptr, indices, data, rows = _lap()
    bt = _vectors()[1]
    s = _pow2_scale(N, block)
    assert len(set(s[N_STRIDED:].tolist())) == 7 and len(set(s[N - 13:].tolist())) > 1
    xs = []
    for vals, b in ((data, bt), (s[rows] * data * s[indices], s * bt)):
        with _bj_context(gpu_pkg, p, (indptr, indices, vals), block) as c:
            x, res = _run(c, b, iters)
            assert res["iterations"] == iters and res["converged"] == 0, res
            xs.append(x)
    xt, xj = xs
    assert np.all(np.isfinite(xt)) and np.all(np.isfinite(xj)) and np.linalg.norm(xt) > 0
    sx = s * xj
    same = np.array_equal(sx.view(np.uint64), xt.view(np.uint64))
    bad = np.flatnonzero(sx != xt)
    print("scaled block %d p=%d: same=%s |s x_S - x| / |x| = %.3e, %d rows differ (first %s, %d of them from row %d on)" % (
        block, p, same, _rel(sx, xt), len(bad), bad[:1].tolist(), int(np.count_nonzero(bad >= N_STRIDED)), N_STRIDED))
    assert same, (block, p, len(bad))


def _block_diagonal_csr(n, block, seed):
    """ref.block_diagonal_matrix's blocks M M^T + m I (every block its own M), built straight into CSR.  Returns (csr, b)."""
    rng = np.random.default_rng(seed)
    nb, m = n // block, n % block
    M = rng.standard_normal((nb, block, block))
    D = M @ M.transpose(0, 2, 1) + block * np.eye(block)
    D = 0.5 * (D + D.transpose(0, 2, 1))
    Mt = rng.standard_normal((m, m))
    Dt = Mt @ Mt.T + m * np.eye(m)
    Dt = 0.5 * (Dt + Dt.T)
    data = np.concatenate([D.reshape(-1), Dt.reshape(-1)])
    first = np.arange(n) // block * block                      # the first column of row i's block
    cols = np.concatenate([(first[:nb * block, None] + np.arange(block)[None, :]).reshape(-1),
                           (first[nb * block:, None] + np.arange(m)[None, :]).reshape(-1)])
    counts = np.concatenate([np.full(nb * block, block), np.full(m, m)])
    indptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    assert len(indptr) == n + 1 and indptr[-1] == len(data) == len(cols) and np.all(data != 0)
    return (indptr, cols.astype(np.int32), data), rng.standard_normal(n)


@pytest.mark.parametrize("p", [1, 3])
@pytest.mark.parametrize("block", [8, 32])
def test_block_jacobi_exact_on_a_block_diagonal_matrix(gpu_pkg, block, p):
    csr, b = _block_diagonal_csr(N, block, 1000 * block + 1)
    assert N % block and not np.array_equal(csr[2][:block * block], csr[2][block * block:2 * block * block])
    with _bj_context(gpu_pkg, p, csr, block) as c:
        x, res = _run(c, b, 1)
        c.set_preconditioner("jacobi")
        assert c.preconditioner_block() == 1
        _, point = _run(c, b, 1)
    host = float(np.linalg.norm(lv.matvec(*csr, x) - b) / np.linalg.norm(b))
    print("block diagonal %d p=%d: rel_residual %.3e after one iteration, host %.3e (point Jacobi %.3e)" % (
        block, p, res["rel_residual"], host, point["rel_residual"]))
    assert res["iterations"] == 1 and res["rel_residual"] <= 1e-12, res
    assert host <= 1e-12, host
    assert point["rel_residual"] > 1e-3, point


@pytest.mark.parametrize("p", [1, 3])
def test_block_inverses_of_the_second_trip(gpu_pkg, p):
    """Block 32 on S L S: W for every row from 262144 on -- the 42 full blocks of the five full tiles and of the last tile, and
    the truncated block of 13 rows -- on every shard: symmetric bit for bit, zero outside the block, and
    max |W_blk D_blk - I| <= 4 m 2^-52 kappa_2(D_blk) in longdouble (the bar of tests/test_gpu_block_jacobi.py
    test_inverse_alone)."""
    block = 32
    indptr, indices, _, _ = _lap()
    scaled, bs = _sls()
    s = _vectors()[0]
    with _bj_context(gpu_pkg, p, (indptr, indices, scaled), block) as c:
        c.set_max_iter(1)
        c.set_source_term(bs)
        c.solve_begin(np.zeros(N))
        c.solve_end(np.zeros(N))
        Ws = [c._probe_precond_blocks(q) for q in range(p)]
    ranges = [(a, e) for a, e in ref.block_ranges(N, block) if a >= N_STRIDED]
    assert len(ranges) == 43 and ranges[0][0] == N_STRIDED and ranges[-1] == (N - 13, N)
    worst = 0.0
    for q, W in enumerate(Ws):
        assert W.shape == (N, block)
        for a, e in ranges:
            m = e - a
            Wb = W[a:e, :m]
            assert np.array_equal(Wb.view(np.uint64), Wb.T.copy().view(np.uint64)), (q, a, "not symmetric bit for bit")
            assert not W[a:e, m:].any(), (q, a, "not zero outside the block")
            D = s[a:e, None] * lv.toeplitz_block(m) * s[None, a:e]
            err = float(np.max(np.abs(Wb.astype(LD) @ D.astype(LD) - np.eye(m, dtype=LD))))
            bar = 4 * m * EPS * float(np.linalg.cond(D, 2))
            worst = max(worst, err / bar)
            assert err <= bar, (q, a, m, err, bar)
        assert np.array_equal(W.view(np.uint64), Ws[0].view(np.uint64)), (q, "the shards hold different inverses")
    print("inverse block %d p=%d, rows from %d on: worst max|W D - I| / (4 m eps kappa) = %.2e" % (block, p, N_STRIDED, worst))


# ---- multi-shift CG, one GPU ------------------------------------------------------------------------------------------------------
def _shift_context(pkg, variant=0):
    """The generator's matrix at N on CSR storage with the standard-normal source term; the plan asserted."""
    indptr, indices, data, _ = _lap()
    c = tc.solver(pkg, 1, gemv_variant=variant)
    try:
        c.set_matrix_csr(indptr, indices, data)
        c.set_source_term(_vectors()[1])
        plan = c.gemv_plan()
        assert c.n() == N > N_STRIDED and _shards(c) == 1
        assert plan["variant"] == 7 and (variant == 0 or plan["R"] == variant - 70000), plan
    except BaseException:
        c.close()
        raise
    return c


@pytest.mark.parametrize("variant", [0, 70008])
def test_zero_shift_is_the_plain_solve(gpu_pkg, variant):
    b = _vectors()[1]
    with _shift_context(gpu_pkg, variant) as c:
        c.set_max_iter(40)
        c.tolerance(0.0)
        r, res = ts._zero_shift_is_plain_solve(c, N)
        assert r["iterations"] == 40 and r["converged"] == 0, r
        assert res[0]["residual_last"] == r["residual_last"], (res[0], r)
        tol = 1e-2 * float(np.linalg.norm(b))   # the seed's own break
        c.set_max_iter(2000)
        c.tolerance(tol)
        r, res = ts._zero_shift_is_plain_solve(c, N)
        print("zero shift, variant %d: the seed breaks at %d, residual_last %.17g" % (variant, r["iterations"], r["residual_last"]))
        assert r["converged"] == 1 and 0 < r["iterations"] < 2000, r
        assert res[0]["residual_last"] == r["residual_last"] < tol <= r["residual_prev"], (res[0], r)


def test_every_shift_against_longdouble(gpu_pkg):
    iters = 12
    indptr, indices, data, rows = _lap()
    b = _vectors()[1]
    with _shift_context(gpu_pkg) as c:
        c.set_max_iter(iters)
        c.tolerance(0.0)
        X, res = c.solve_shifted(S7)
    assert X.shape == (len(S7), N)
    for j, sigma in enumerate(S7):
        want = _shift_reference(sigma, iters, 0.0)
        err = _rel(X[j], want["x"])
        xn = float(np.linalg.norm(X[j]))
        offs = {k: abs(res[j][k] - want[k]) / want[k] for k in ("residual_prev", "residual_last")}
        print("shift %g: |dx|/|x| = %.2e (bar %.0e), residual_prev off by %.2e, residual_last by %.2e (bar %.0e), x_norm by %.2e" % (
            sigma, err, SHIFT_X_BOUND, offs["residual_prev"], offs["residual_last"], RESIDUAL_BOUND, abs(res[j]["x_norm"] - xn) / xn))
        assert res[j]["iterations"] == want["iterations"] == iters and res[j]["converged"] == 0, (sigma, res[j])
        assert err <= SHIFT_X_BOUND, (sigma, err)
        for k, off in offs.items():
            assert off <= RESIDUAL_BOUND, (sigma, k, res[j][k], want[k])
        assert abs(res[j]["x_norm"] - xn) <= NORM_BOUND * xn, (sigma, res[j]["x_norm"], xn)
        ax, aax = _csr_products(rows, indices, data, X[j], N)
        _check_rel_residual(res[j], ax + sigma * X[j], aax + sigma * np.abs(X[j]), b, 6, sigma)


def test_widths_and_companions(gpu_pkg):
    """The column of sigma = 1 inside S7 (k_shift_update<8>), alone (<1>) and inside 16 shifts (<16>): the same bits and the same
    result tuple; a permutation of S7 permutes the output.  40 iterations at tol = 1e-8: the large shifts freeze on the way."""
    perm = np.random.default_rng(1).permutation(len(S7))
    others = [0.0, 0.5, 2.0, 3.0, 4.0, 5.0, 6.0, 8.0, 9.0, 10.0, 20.0, 50.0, 200.0, 1e3, 1e5]
    with _shift_context(gpu_pkg) as c:
        c.set_max_iter(40)
        c.tolerance(1e-8)
        X, res = c.solve_shifted(S7)
        Xp, resp = c.solve_shifted([S7[q] for q in perm])
        X1, res1 = c.solve_shifted([1.0])
        X16, res16 = c.solve_shifted(others[:7] + [1.0] + others[7:])
    assert len(others) == 15 and np.isfinite(X).all() and np.linalg.norm(X[S7.index(1.0)]) > 0
    frozen = [r["converged"] for r in res]
    print("widths: converged %s, iterations %s" % (frozen, [r["iterations"] for r in res]))
    assert frozen[S7.index(1e4)] == 1 and frozen[0] == 0, res
    assert np.array_equal(Xp, X[perm])
    assert ts._tuples(resp) == [ts._tuples(res)[q] for q in perm]
    j = S7.index(1.0)
    assert np.array_equal(X1[0], X[j]) and np.array_equal(X16[7], X[j])
    assert ts._tuples(res1)[0] == ts._tuples(res)[j] == ts._tuples(res16)[7]


def test_a_frozen_shift_stays_frozen_in_the_second_trip(gpu_pkg):
    """Shifts 100 and 1e4 freeze after a few iterations while the seed runs on to max_iter = 60: from then on k_shift_update's
    second loop must leave their rows from 262144 on alone as the first trip leaves the rows below."""
    shifts, tol, iters = [0.0, 100.0, 1e4], 1e-10, 60
    with _shift_context(gpu_pkg) as c:
        c.set_max_iter(iters)
        c.tolerance(tol)
        x = np.zeros(N)
        r = c.solve(x)
        X, res = c.solve_shifted(shifts)
    assert r["converged"] == 0 and r["iterations"] == iters and r["residual_last"] > 1e6 * tol, r   # the seed is far from done
    assert np.array_equal(X[0], x) and res[0]["iterations"] == iters and res[0]["converged"] == 0
    assert res[0]["residual_prev"] == r["residual_prev"] and res[0]["residual_last"] == r["residual_last"]
    for j in (1, 2):
        want = _shift_reference(shifts[j], iters, tol)
        k = res[j]["iterations"]
        print("frozen sigma=%g: stops at %d (reference %d)" % (shifts[j], k, want["iterations"]))
        assert want["converged"] == 1 and want["iterations"] < 20
        assert res[j]["converged"] == 1 and abs(k - want["iterations"]) <= 1, (res[j], want["iterations"])
        xr = _shift_reference(shifts[j], 24, 0.0, tuple(range(1, 25)))["xs"][k + 1]   # x after k + 1 updates
        low, high = _rel(X[j][:N_STRIDED], xr[:N_STRIDED]), _rel(X[j][N_STRIDED:], xr[N_STRIDED:])
        print("frozen sigma=%g: |dx|/|x| rows below %d: %.2e, rows from there on: %.2e (bar %.0e)" % (
            shifts[j], N_STRIDED, low, high, SHIFT_X_BOUND))
        assert low <= SHIFT_X_BOUND and high <= SHIFT_X_BOUND, (shifts[j], low, high)
