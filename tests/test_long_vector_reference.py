"""tests/long_vector_reference.py pinned on the CPU, before tests/test_gpu_long_vectors.py leans on it.

1. pcg_scaled_lap2d (ONE Toeplitz inverse, applied as s^-1 T^-1 s^-1) against references that form every block inverse from the
   actual block of S L S, in longdouble over 12 iterations, 1e-13 relative, for blocks 4, 32 and 256.  The identity needs
   block <= inc = floor(sqrt(n)) and the helper asserts it, so each block size gets the smallest kind of n that allows it:
   block 4 at n = 1000 and 1001 and block 32 at n = 1101 (inc = 33, n mod 32 = 13) against ref.pcg on the dense matrix; block 256 needs
   n >= 65536, where no dense matrix fits, so at n = 66125 (inc = 257, n mod 256 = 77) the reference solves with every actual
   block (tridiagonal: checked entry by entry) by the Thomas algorithm -- and that reference is itself tied to ref.pcg in the two
   dense cases.  Measured: 2.3e-17 and 2.7e-17 (block 4), 2.7e-17 (block 32) against ref.pcg,
   6.2e-18 (block 256) against the Thomas reference, which is itself within 2.7e-17 of ref.pcg.
2. cg_shifted against oracle.solve(A + sigma I, b) at n = 1000 for the shifts of tests/test_gpu_shifted.py S7: 12 iterations at
   tol = 0 (x to 1e-12, the reported residuals to 1e-9: the project's bars for these quantities on the GPU), and the stop at
   tol = 1e-10 for the two large shifts.  Measured: x at most 2.1e-14 (sigma = 1e-3), the residuals at most 1.4e-11
   (sigma = 1e4; 2.5e-13 at sigma = 100, at most 2.5e-14 elsewhere); both stop where the oracle stops, at 8 and 3.
3. At n = N_LONG = 263501 the fp64 run of each reference against its longdouble run, 12 iterations, b standard normal,
   s = geomspace(1, 100) permuted: each distance must be at most a quarter of the GPU bar it supports (1e-10 for the block-Jacobi
   x, 1e-12 for the shifted x, 1e-9 for the shifted residuals).  Measured: 6.7e-16, 4.2e-16 and 4.2e-16 for blocks 4, 32 and 256;
   over S7 at most 4.2e-15 in x and 6.0e-15 in the residuals.
   For blocks 4 and 32 the fp64 inverses are also formed from the actual blocks S_b T S_b (Gauss-Jordan without pivoting as
   ref.invert_spd does it, all blocks at once; sampled blocks equal ref.invert_spd(..., np.float64) bit for bit): what inverting
   the scaled block rather than T costs.  Measured: 4.3e-16 (block 4) and 4.8e-16 (block 32), i.e. nothing beyond the fp64 level
   of the line above.
4. The fault the GPU tests are after, modelled in numpy: a block inverse taken from the first trip's tile for the rows from
   262144 on changes nothing on the generator's matrix (0 exactly) and 0.97 relative on S L S."""
import functools

import numpy as np
import pytest

import block_jacobi_reference as ref
import long_vector_reference as lv

LD = np.longdouble
S7 = [0.0, 1e-3, 0.05, 1.0, 7.5, 100.0, 1e4]   # tests/test_gpu_shifted.py
N = lv.N_LONG
ITERS = 12
BJ_BAR, SHIFT_X_BAR, SHIFT_RES_BAR = 1e-10, 1e-12, 1e-9   # the GPU bars of tests/test_gpu_long_vectors.py


def _rel(a, b):
    a, b = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def test_the_size():
    assert N == 263501 and N > lv.N_STRIDED == 256 * 1024
    assert -(-N // 256) == 1030 and N % 256 == 77 and N % 32 == 13 and N % 4 == 1 and N % 2 == 1
    assert all((q * (N // 3)) % 256 for q in (1, 2))   # the shard boundaries cut tiles (and so blocks of 256)
    assert int(np.floor(np.sqrt(N))) == 513


def test_matvec_against_dense():
    n = 1000
    indptr, indices, data = lv.tc.lap2d_csr(n)
    A = lv.tc.csr_to_dense(indptr, indices, data, n)
    x = lv.normal_b(n)
    got, want = lv.matvec(indptr, indices, data.astype(LD), x.astype(LD)), A.astype(LD) @ x.astype(LD)
    bound = 5 * np.finfo(LD).eps * (np.abs(A) @ np.abs(x))   # two orders of a sum of at most 5 terms
    assert got.dtype == LD and np.all(np.abs(got - want) <= bound)
    with pytest.raises(AssertionError):   # an empty row would shift every later row of reduceat
        lv.matvec(np.array([0, 1, 1, 2]), np.array([0, 2]), np.ones(2), np.ones(3))


# ---- 1. pcg_scaled_lap2d against inverses of the actual blocks -----------------------------------------------------------------
def _thomas_apply(csr, n, block, dtype):
    """z = D_b^-1 r from the actual entries of every diagonal block, which must be tridiagonal: Thomas, all blocks at once."""
    indptr, indices, data = csr
    rows = lv.csr_rows(indptr)
    inblock = rows // block == indices // block
    assert np.all(np.abs(rows - indices)[inblock] <= 1), "a diagonal block is not tridiagonal"
    nbt = -(-n // block)
    d = np.ones(nbt * block, dtype=dtype)
    e = np.zeros(nbt * block, dtype=dtype)                  # e[i] = A(i, i + 1) inside the block
    low = np.zeros(nbt * block, dtype=dtype)                # low[i] = A(i, i - 1) inside the block
    dm, um, lm = indices == rows, inblock & (indices == rows + 1), inblock & (indices == rows - 1)
    d[rows[dm]], e[rows[um]], low[rows[lm]] = data[dm], data[um], data[lm]
    assert np.array_equal(e[:-1][e[:-1] != 0], low[1:][low[1:] != 0])   # symmetric
    d, e = d.reshape(nbt, block), e.reshape(nbt, block)

    def apply_z(r):
        rp = np.zeros(nbt * block, dtype=dtype)
        rp[:n] = r
        rp = rp.reshape(nbt, block)
        dp = d.copy()
        for t in range(1, block):
            w = e[:, t - 1] / dp[:, t - 1]
            dp[:, t] -= w * e[:, t - 1]
            rp[:, t] -= w * rp[:, t - 1]
        z = np.empty_like(rp)
        z[:, -1] = rp[:, -1] / dp[:, -1]
        for t in range(block - 2, -1, -1):
            z[:, t] = (rp[:, t] - e[:, t] * z[:, t + 1]) / dp[:, t]
        return z.reshape(-1)[:n].copy()

    return apply_z


@pytest.mark.parametrize("n,block", [(1000, 4), (1001, 4), (1101, 32), (66125, 256)])
def test_scaled_lap2d_pcg_against_inverses_of_the_actual_blocks(n, block):
    inc = int(np.floor(np.sqrt(n)))
    assert block <= inc and (n % block or n == 1000) and (block < 256 or n % 256 == 77)
    s = lv.spread_scale(n)
    bs = s * lv.normal_b(n)
    got = lv.pcg_scaled_lap2d(n, s, bs, block, ITERS, LD)
    assert got["iterations"] == ITERS and got["converged"] == 0
    csr = lv.scaled_lap2d(n, s, LD)
    thomas = lv.pcg_csr(csr, bs, _thomas_apply(csr, n, block, LD), ITERS, 0.0, LD)
    err = _rel(got["x"], thomas["x"])
    print("block %d n=%d: |x - x_thomas| / |x| = %.3e" % (block, n, err))
    assert err <= 1e-13
    assert abs(got["residual_last"] - thomas["residual_last"]) <= 1e-13 * thomas["residual_last"]
    if n <= 2000:
        L = lv.tc.csr_to_dense(*lv.tc.lap2d_csr(n), n)
        sl = s.astype(LD)
        dense = ref.pcg((sl[:, None] * L.astype(LD)) * sl[None, :], bs, block, ITERS, 0.0, LD)
        err_d, err_t = _rel(got["x"], dense["x"]), _rel(thomas["x"], dense["x"])
        print("block %d n=%d: |x - x_dense| / |x| = %.3e (Thomas against dense %.3e)" % (block, n, err_d, err_t))
        assert err_d <= 1e-13 and err_t <= 1e-13
        assert abs(got["residual_last"] - dense["residual_last"]) <= 1e-13 * dense["residual_last"]
        assert abs(got["residual_prev"] - dense["residual_prev"]) <= 1e-13 * dense["residual_prev"]


def test_the_identity_is_refused_where_the_far_diagonals_enter_a_block():
    n = 1000   # inc = 31
    with pytest.raises(AssertionError):
        lv.pcg_scaled_lap2d(n, np.ones(n), np.ones(n), 32, 1)
    with pytest.raises(AssertionError):   # and the Thomas reference sees the far diagonal inside a block of 64
        _thomas_apply(lv.tc.lap2d_csr(n), n, 64, LD)


# ---- 2. cg_shifted against the oracle on the shifted dense matrix ------------------------------------------------------------------
def test_shifted_cg_against_oracle(oracle):
    n = 1000
    csr = lv.tc.lap2d_csr(n)
    A = oracle.generate_lap2d(n)
    assert np.array_equal(lv.tc.csr_to_dense(*csr, n), A)
    b = oracle.init_source_term(n)
    worst = [0.0, 0.0]
    for sigma in S7:
        xo, ro = oracle.solve(A + sigma * np.eye(n), b, max_iter=ITERS, tol=0.0)
        got = lv.cg_shifted(csr, b, sigma, ITERS, 0.0, LD)
        ex = _rel(got["x"], xo)
        er = max(abs(got[k] - ro[k]) / ro[k] for k in ("residual_prev", "residual_last"))
        worst = [max(worst[0], ex), max(worst[1], er)]
        print("sigma=%g: |dx|/|x| = %.3e, residuals %.3e" % (sigma, ex, er))
        assert got["iterations"] == ro["iterations"] == ITERS and got["converged"] == ro["converged"] == 0
        assert ex <= SHIFT_X_BAR and er <= SHIFT_RES_BAR, (sigma, ex, er)
    print("worst over S7: x %.3e, residuals %.3e" % tuple(worst))
    for sigma in (100.0, 1e4):   # the stop, counted as the library counts it
        xo, ro = oracle.solve(A + sigma * np.eye(n), b, max_iter=n, tol=1e-10)
        got = lv.cg_shifted(csr, b, sigma, n, 1e-10, LD, keep=range(1, 40))
        print("sigma=%g: stops at %d (oracle %d), residual_last %.3e / %.3e" % (sigma, got["iterations"], ro["iterations"],
                                                                               got["residual_last"], ro["residual_last"]))
        assert got["converged"] == ro["converged"] == 1 and got["iterations"] == ro["iterations"] < 20
        assert got["residual_last"] < 1e-10 <= got["residual_prev"]
        assert abs(got["residual_prev"] - ro["residual_prev"]) <= SHIFT_RES_BAR * ro["residual_prev"]
        assert np.array_equal(got["xs"][got["iterations"] + 1], got["x"])   # x after iterations + 1 updates
        assert _rel(got["x"], xo) <= SHIFT_X_BAR


# ---- 3. fp64 against longdouble at the size of the GPU tests --------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _problem():
    s, b = lv.spread_scale(N), lv.normal_b(N)
    for a in (s, b):
        a.setflags(write=False)
    return s, b


def _invert_all(D):
    """ref.invert_spd on a stack of blocks (nb, m, m), in D's precision: the same operations in the same order per block."""
    a = D.copy()
    nb, m, _ = a.shape
    inv = np.broadcast_to(np.eye(m, dtype=a.dtype), a.shape).copy()
    for k in range(m):
        p = a[:, k, k].copy()
        a[:, k] /= p[:, None]
        inv[:, k] /= p[:, None]
        f = a[:, :, k].copy()
        f[:, k] = 0
        a -= f[:, :, None] * a[:, k][:, None, :]
        inv -= f[:, :, None] * inv[:, k][:, None, :]
    return inv


@pytest.mark.parametrize("block", [4, 32, 256])
def test_fp64_block_jacobi_reference_is_far_inside_the_gpu_bar(block):
    s, b = _problem()
    old = lv.pcg_scaled_lap2d(N, s, s * b, block, ITERS, LD)
    new = lv.pcg_scaled_lap2d(N, s, s * b, block, ITERS, np.float64)
    err = _rel(new["x"], old["x"])
    print("block %d n=%d: fp64 against longdouble |dx|/|x| = %.3e (a quarter of the bar: %.1e)" % (block, N, err, BJ_BAR / 4))
    assert err <= BJ_BAR / 4
    if block == 256:
        return
    # the inverses from the actual fp64 blocks S_b T S_b, as the library forms them
    nb, m = N // block, N % block
    sh = s[:nb * block].reshape(nb, block)
    full = _invert_all(sh[:, :, None] * lv.toeplitz_block(block)[None] * sh[:, None, :])
    st = s[nb * block:]
    Dt = st[:, None] * lv.toeplitz_block(m) * st[None, :]
    tail = ref.invert_spd(Dt, np.float64)
    for j in (0, nb // 2, nb - 1):
        D = s[j * block:(j + 1) * block, None] * lv.toeplitz_block(block) * s[None, j * block:(j + 1) * block]
        assert np.array_equal(full[j], ref.invert_spd(D, np.float64)), j
    act = lv.pcg_csr(lv.scaled_lap2d(N, s), s * b, lambda r: lv.blockwise(N, block, r, full, tail), ITERS, 0.0, np.float64)
    err_a = _rel(act["x"], old["x"])
    print("block %d n=%d: fp64 inverses of the actual blocks against longdouble |dx|/|x| = %.3e" % (block, N, err_a))
    assert err_a <= BJ_BAR / 4


def test_an_inverse_of_the_wrong_tile_shows_on_the_scaled_matrix_only():
    """The fault the GPU tests are after, modelled here: rows from 262144 on apply the block inverse of the same row of the first
    trip's tile (row i - 262144).  On the generator's matrix every full block is the same, so x does not move at all; on S L S
    with s differing from row to row it moves by far more than the bar."""
    block = 4
    s, b = _problem()
    src = np.arange(N)
    src[lv.N_STRIDED:] -= lv.N_STRIDED
    assert lv.N_STRIDED % block == 0 and np.count_nonzero(src != np.arange(N)) == N - lv.N_STRIDED
    full = ref.invert_spd(lv.toeplitz_block(block), np.float64)
    tail = ref.invert_spd(lv.toeplitz_block(N % block), np.float64)
    for name, sv, bound in (("generator", np.ones(N), None), ("scaled", s, 1e4 * BJ_BAR)):
        sw = sv[src]
        good = lv.pcg_scaled_lap2d(N, sv, sv * b, block, ITERS, np.float64)
        bad = lv.pcg_csr(lv.scaled_lap2d(N, sv), sv * b, lambda r: lv.blockwise(N, block, r / sw, full, tail) / sw, ITERS, 0.0,
                         np.float64)
        err = _rel(bad["x"], good["x"])
        print("wrong tile, %s matrix: |dx|/|x| = %.3e" % (name, err))
        assert (err == 0.0) if bound is None else (err >= bound), (name, err)


def test_fp64_shifted_reference_is_far_inside_the_gpu_bars():
    _, b = _problem()
    csr = lv.tc.lap2d_csr(N)
    worst = [0.0, 0.0]
    for sigma in S7:
        old = lv.cg_shifted(csr, b, sigma, ITERS, 0.0, LD)
        new = lv.cg_shifted(csr, b, sigma, ITERS, 0.0, np.float64)
        ex = _rel(new["x"], old["x"])
        er = max(abs(new[k] - old[k]) / old[k] for k in ("residual_prev", "residual_last"))
        worst = [max(worst[0], ex), max(worst[1], er)]
        print("sigma=%g n=%d: fp64 against longdouble |dx|/|x| = %.3e, residuals %.3e" % (sigma, N, ex, er))
    print("worst over S7: x %.3e (a quarter of the bar: %.1e), residuals %.3e (%.1e)" % (worst[0], SHIFT_X_BAR / 4, worst[1],
                                                                                       SHIFT_RES_BAR / 4))
    assert worst[0] <= SHIFT_X_BAR / 4 and worst[1] <= SHIFT_RES_BAR / 4
