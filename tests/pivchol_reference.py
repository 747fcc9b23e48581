"""numpy restatement of the pivoted-Cholesky preconditioner for tests/test_pivchol_abi.py and
tests/test_gpu_pivchol.py: the kernel matrices of the issue's recipe, the set-up, the Woodbury apply and the PCG recurrence of
section 11, each in the dtype it is given (float64 or longdouble).  Not a test module and not part of the product."""
import functools

import numpy as np

LD = np.longdouble
EPS = 2.0 ** -52


@functools.lru_cache(maxsize=None)
def kernel_matrix(n, ell, sigma2, seed=20261018):
    """A = S K S + sigma^2 I, K_ij = exp(-|x_i - x_j|^2 / (2 ell^2)), points uniform in [0, 1]^2, s_i log-uniform in [1, 4];
    b_i = sin(0.37 i) + 0.5.  Returns (A, b), read-only."""
    rng = np.random.default_rng(seed)
    pts = rng.random((n, 2))
    s = np.exp(rng.uniform(0.0, np.log(4.0), n))
    d2 = ((pts[:, None, :] - pts[None, :, :]) ** 2).sum(axis=2)
    A = s[:, None] * np.exp(-d2 / (2.0 * ell * ell)) * s[None, :]
    A = 0.5 * (A + A.T)
    A[np.diag_indices(n)] += sigma2
    b = np.sin(0.37 * np.arange(n)) + 0.5
    A.setflags(write=False)
    b.setflags(write=False)
    return A, b


def pivoted_cholesky(A, rank, shift=0.0):
    """The set-up in float64: (pivots, L (n x rank), delta, remaining diagonal with -inf at the chosen rows).  Step t: the pivot
    is the not yet chosen row with the largest remaining diagonal (np.argmax: ties to the smallest index);
    l_i = (A[p][i] - sum_{u<t} L[i][u] L[p][u]) / sqrt(d_p), exactly sqrt(d_p) at p and 0 at rows chosen earlier."""
    n = A.shape[0]
    d = np.array(np.diag(A), dtype=np.float64)
    L = np.zeros((n, rank))
    piv = np.zeros(rank, dtype=np.int64)
    for t in range(rank):
        p = int(np.argmax(d))
        dp = d[p]
        assert np.isfinite(dp) and dp > 0.0, (t, p, dp)
        piv[t] = p
        sq = np.sqrt(dp)
        l = (A[p, :] - L[:, :t] @ L[p, :t]) / sq
        l[d == -np.inf] = 0.0
        l[p] = sq
        L[:, t] = l
        d = np.where(d == -np.inf, d, d - l * l)
        d[p] = -np.inf
    delta = float(shift) if shift > 0.0 else float(np.where(d == -np.inf, 0.0, d).sum() / n)
    return piv, L, delta, d


def remaining_diagonal_checks(A, piv, L):
    """From A and the returned columns 0 ... t-1, in longdouble: (the smallest ratio of a pivot's remaining diagonal to the
    largest remaining one over the steps, the mean remaining diagonal after the last step)."""
    n = A.shape[0]
    d = np.diag(A).astype(LD)
    free = np.ones(n, dtype=bool)
    worst = LD(np.inf)
    for t, p in enumerate(piv):
        best = d[free].max()
        worst = min(worst, d[p] / best)
        free[p] = False
        d = d - L[:, t].astype(LD) ** 2
    return float(worst), d[free].sum() / LD(n) if free.any() else LD(0)


def pivot_row_error(A, piv, L):
    """max |A[p_t, :] - (L L^T)[p_t, :]| over the pivot rows, in longdouble."""
    Lp = L[np.asarray(piv)].astype(LD)
    return float(np.abs(A[np.asarray(piv)].astype(LD) - Lp @ L.astype(LD).T).max())


def _chol_factor(C):
    """The lower Cholesky factor of SPD C, unpivoted, in C's dtype (np.linalg has no longdouble)."""
    k = C.shape[0]
    R = np.array(C, copy=True)
    for j in range(k):
        R[j, j] = np.sqrt(R[j, j] - R[j, :j] @ R[j, :j])
        if j + 1 < k:
            R[j + 1:, j] = (R[j + 1:, j] - R[j + 1:, :j] @ R[j, :j]) / R[j, j]
    return R


def _chol_solve(R, t):
    y = np.array(t, dtype=R.dtype, copy=True)
    k = R.shape[0]
    for j in range(k):
        y[j] = (y[j] - R[j, :j] @ y[:j]) / R[j, j]
    for j in range(k - 1, -1, -1):
        y[j] = (y[j] - R[j + 1:, j] @ y[j + 1:]) / R[j, j]
    return y


class Woodbury:
    """z = (r - L (delta I + L^T L)^-1 L^T r) / delta in `dtype`, from a given L and delta."""

    def __init__(self, L, delta, dtype):
        self.L = np.asarray(L).astype(dtype)
        self.delta = dtype(delta)
        self.dtype = dtype
        k = self.L.shape[1]
        self.C = self.L.T @ self.L + self.delta * np.eye(k, dtype=dtype)
        self.R = _chol_factor(self.C)

    def apply(self, r):
        r = np.asarray(r).astype(self.dtype)
        return (r - self.L @ _chol_solve(self.R, self.L.T @ r)) / self.delta


def pcg(A, b, apply, tol, max_iter, dtype):
    """The library's PCG from a zero guess with z = apply(r): the break on sqrt(r.r) < tol is taken at the
    head of iteration k + 1, `iterations` = k.  Returns iterations, converged, x and the history of sqrt(r.r)."""
    A = np.asarray(A).astype(dtype)
    x = np.zeros(len(b), dtype=dtype)
    r = np.asarray(b).astype(dtype).copy()
    z = apply(r)
    p = z.copy()
    rho = r @ z
    hist = [float(np.sqrt(r @ r))]
    for k in range(max_iter):
        Ap = A @ p
        alpha = rho / (p @ Ap)
        x = x + alpha * p
        r = r - alpha * Ap
        hist.append(float(np.sqrt(r @ r)))
        if hist[-1] < tol:
            return {"iterations": k, "converged": 1, "x": x, "hist": hist}
        z = apply(r)
        rho_new = r @ z
        p = z + (rho_new / rho) * p
        rho = rho_new
    return {"iterations": max_iter, "converged": 0, "x": x, "hist": hist}
