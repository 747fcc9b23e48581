"""Sparse host references for the long-vector tests (tests/test_gpu_long_vectors.py, pinned by tests/test_long_vector_reference.py):
the library's recurrence and stopping rule as tests/block_jacobi_reference.py pcg states them, on a CSR matrix in numpy, in
np.longdouble or np.float64.  No scipy.

- matvec: one CSR product.
- cg_shifted: plain CG on A + sigma I (multi-shift CG's answer for one shift).
- pcg_scaled_lap2d: block-Jacobi PCG on A = S L S, L the generator's lap2d and S = diag(s), without forming n / block inverses:
  the off-diagonals of L at +-(inc + 1) lie outside every diagonal block of size <= inc, so D_b(A) = S_b T S_b with T the
  tridiagonal Toeplitz block (4, -1) and z = s^-1 T^-1 (s^-1 r) block by block."""
import numpy as np

import block_jacobi_reference as ref
import test_gpu_csr as tc


N_STRIDED = 262144                 # 256 * kMaxVectorGrid (cgx_kernels.h): above it the update kernels stride over the rows
N_LONG = 262144 + 5 * 256 + 77     # 263501: 1030 tiles on 1024 workgroups (workgroups 0 - 5 take a second trip), 77 rows in the
                                   # last tile, odd (n mod 256 = 77, n mod 32 = 13, n mod 4 = 1: the last block is truncated for
                                   # every block size), and n / 3 cuts blocks and tiles at shard boundaries
SEED = 20261018


def spread_scale(n, seed=SEED):
    """s spread over [1, 100], permuted: differs from row to row, no power of two."""
    return np.random.default_rng(seed).permutation(np.geomspace(1.0, 100.0, n))


def normal_b(n, seed=SEED + 1):
    return np.random.default_rng(seed).standard_normal(n)


def csr_rows(indptr):
    return np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))


def matvec(indptr, indices, data, x):
    """A x, each row summed on its own in the precision of data and x.  Every row stores at least one entry."""
    assert np.all(np.diff(indptr) > 0) and indptr[0] == 0 and indptr[-1] == len(data)
    return np.add.reduceat(data * x[indices], indptr[:-1])


def pcg_csr(csr, b, apply_z, iters, tol=0.0, dtype=np.longdouble, keep=()):
    """ref.pcg on a CSR matrix with z = apply_z(r).  Returns the same dict: x (fp64), iterations as the library counts them (the
    index of the iteration whose update brought sqrt(r.r) below tol, else iters), converged, residual_prev / residual_last
    (sqrt(r.r) before / after the last update) and xs[k] = x after k updates for k in keep."""
    indptr, indices, data = csr
    data = np.asarray(data).astype(dtype)
    b = np.asarray(b).astype(dtype)
    x = np.zeros_like(b)
    r = b.copy()
    z = apply_z(r)
    p = z.copy()
    rho = r @ z
    prev = np.sqrt(r @ r)
    out = {"xs": {}, "converged": 0, "iterations": iters}
    last = prev
    for k in range(iters):
        Ap = matvec(indptr, indices, data, p)
        alpha = rho / (p @ Ap)
        x += alpha * p
        r -= alpha * Ap
        last = np.sqrt(r @ r)
        if k + 1 in keep:
            out["xs"][k + 1] = x.astype(np.float64)
        if last < tol:
            out.update(converged=1, iterations=k)
            break
        prev = last
        z = apply_z(r)
        rn = r @ z
        p = z + (rn / rho) * p
        rho = rn
    out.update(x=x.astype(np.float64), residual_prev=float(prev), residual_last=float(last))
    return out


def shifted_data(csr, sigma, dtype=np.float64):
    """The stored values with sigma added to the stored diagonal (every row must store one)."""
    indptr, indices, data = csr
    diag = indices == csr_rows(indptr)
    assert int(diag.sum()) == len(indptr) - 1, "a row without a stored diagonal entry"
    out = np.asarray(data).astype(dtype)
    out[diag] += dtype(sigma)
    return out


def cg_shifted(csr, b, sigma, iters, tol=0.0, dtype=np.longdouble, keep=()):
    """Plain CG on A + sigma I from x0 = 0.  Returns pcg_csr's dict (x, iterations, residual_prev, residual_last, ...)."""
    indptr, indices, _ = csr
    return pcg_csr((indptr, indices, shifted_data(csr, sigma, dtype)), b, lambda r: r.copy(), iters, tol, dtype, keep)


def toeplitz_block(m):
    """The m x m diagonal block of lap2d for m <= inc: tridiagonal (4, -1)."""
    return 4.0 * np.eye(m) - np.eye(m, k=1) - np.eye(m, k=-1)


def scaled_lap2d(n, s, dtype=np.float64):
    """S L S as CSR: (indptr, indices, s[row] * v * s[col])."""
    indptr, indices, data = tc.lap2d_csr(n)
    s = np.asarray(s).astype(dtype)
    return indptr, indices, s[csr_rows(indptr)] * data.astype(dtype) * s[indices]


def blockwise(n, block, r, full, tail):
    """z = D^-1 r for block inverses given as `full` ((block, block): one symmetric inverse shared by all full blocks, or
    (n // block, block, block): one per block) and `tail` (the truncated last block's, or None where block divides n)."""
    nb = n // block
    z = np.empty_like(r)
    head = r[:nb * block].reshape(nb, block)
    if full.ndim == 2:
        z[:nb * block] = (head @ full).reshape(-1)          # full is symmetric: row vectors times T^-1
    else:
        z[:nb * block] = np.einsum("bij,bj->bi", full, head).reshape(-1)
    if n % block:
        z[nb * block:] = tail @ r[nb * block:]
    return z


def pcg_scaled_lap2d(n, s, b, block, iters, dtype=np.longdouble, keep=()):
    """Block-Jacobi PCG on S L S, L = lap2d_csr(n), S = diag(s), s > 0: z = s^-1 T^-1 (s^-1 r) with ONE inverse of the Toeplitz
    block and one of its truncation to n mod block rows."""
    inc = int(np.floor(np.sqrt(n)))
    assert 1 < block <= inc, (block, inc)   # the +-(inc + 1) off-diagonals stay outside every diagonal block
    assert np.all(np.asarray(s) > 0)
    sd = np.asarray(s).astype(dtype)
    full = ref.invert_spd(toeplitz_block(block), dtype)
    tail = ref.invert_spd(toeplitz_block(n % block), dtype) if n % block else None

    def apply_z(r):
        return blockwise(n, block, r / sd, full, tail) / sd

    return pcg_csr(scaled_lap2d(n, s, dtype), b, apply_z, iters, 0.0, dtype, keep)
