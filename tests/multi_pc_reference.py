"""numpy references for tests/test_gpu_multi_pc.py (cgx_solve_multi_pc): the right-hand-side blocks of the
tests, the scaled Laplacian of the Jacobi tests, and the library's PCG (section 11) with an initial guess, column by column, in
the dtype it is given.  Not a test module and not part of the product."""
import numpy as np

LD = np.longdouble


def rhs_block(A, b, k, seed=7):
    """k right-hand sides for the matrix A: b, cos(0.11 i), seeded normal, A (seeded normal), then scaled normals."""
    n = len(b)
    rng = np.random.default_rng(seed)
    i = np.arange(n, dtype=np.float64)
    cols = [np.array(b, dtype=np.float64), np.cos(0.11 * i), rng.standard_normal(n), np.asarray(A) @ rng.standard_normal(n)]
    while len(cols) < k:
        cols.append(rng.standard_normal(n) * (1.0 + len(cols)))
    return np.array(cols[:k])


def x0_block(n, k):
    """Zero guesses, but for column 1."""
    X0 = np.zeros((k, n))
    if k > 1:
        X0[1] = np.sin(np.arange(n) * 0.01)
    return X0


def scaled_lap2d(lap, seed=20261015):
    """S L S with s spread over [1, 100] (geometric, permuted): the matrix of the non-uniform Jacobi tests."""
    n = lap.shape[0]
    s = np.geomspace(1.0, 100.0, n)[np.random.default_rng(seed).permutation(n)]
    return (s[:, None] * lap) * s[None, :]


class CsrOp:
    """The non-zeros of a dense matrix with none of its rows empty, row by row in ascending columns: `op @ v` sums every row in
    that order in the operator's dtype (a longdouble product with a 5-point matrix need not visit a million zeros)."""

    def __init__(self, A, dtype=np.float64):
        A = np.asarray(A)
        rows, self.cols = np.nonzero(A)
        self.vals = A[rows, self.cols].astype(dtype)
        self.ptr = np.flatnonzero(np.r_[True, rows[1:] != rows[:-1]])
        assert len(self.ptr) == A.shape[0]
        self.dense = A

    def astype(self, dtype):
        return CsrOp(self.dense, dtype)

    def __matmul__(self, v):
        return np.add.reduceat(self.vals * v[self.cols], self.ptr)


def jacobi_apply(A, dtype):
    dinv = dtype(1) / np.diag(np.asarray(A)).astype(dtype)
    return lambda r: dinv * r


def pcg_x0(A, b, x0, apply, tol, max_iter, dtype):
    """pivchol_reference.pcg with an initial guess: the library's PCG with z = apply(r), p0 = z0,
    alpha = r.z / p.Ap, beta = r.z(new) / r.z(old); the break on sqrt(r.r) < tol is taken at the head of iteration k + 1,
    `iterations` = k.  A is taken in the dtype it has.  Returns iterations, converged, x, hist (sqrt(r.r) behind the set-up and
    behind every update) and rel_residual = ||A x - b|| / ||b||."""
    b = np.asarray(b).astype(dtype)
    x = np.asarray(x0).astype(dtype).copy()
    r = b - A @ x
    z = apply(r)
    p = z.copy()
    rho = r @ z
    hist = [float(np.sqrt(r @ r))]
    out = {"iterations": max_iter, "converged": 0}
    for k in range(max_iter):
        Ap = A @ p
        alpha = rho / (p @ Ap)
        x = x + alpha * p
        r = r - alpha * Ap
        hist.append(float(np.sqrt(r @ r)))
        if hist[-1] < tol:
            out = {"iterations": k, "converged": 1}
            break
        z = apply(r)
        rho_new = r @ z
        p = z + (rho_new / rho) * p
        rho = rho_new
    d = A @ x - b
    out.update(x=x, hist=hist, rel_residual=float(np.sqrt(d @ d) / np.sqrt(b @ b)))
    return out


def pcg_block(A, B, X0, apply, tol, max_iter, dtype):
    """pcg_x0 for every row of B (k, n) from the guesses X0 (k, n): the columns are independent, each with its own break."""
    Ad = A.astype(dtype)                                    # (an array or a CsrOp)
    return [pcg_x0(Ad, B[j], X0[j], apply, tol, max_iter, dtype) for j in range(B.shape[0])]
