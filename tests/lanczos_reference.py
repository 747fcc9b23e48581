"""Host restatements for the Lanczos quadrature tests (tests/test_lanczos_abi.py, tests/test_gpu_lanczos.py): the recurrence of
csrc/cgx_lanczos.hip in float64 numpy, a longdouble Lanczos with full reorthogonalisation as the high-precision reference, Gauss
quadrature through numpy.linalg.eigh of the dense Jacobi matrix, the library's Rademacher probes, the tolerance rule, and a
matrix-free generate_lap2d_matrix for the sizes of tests/test_gpu_lanczos_tiles.py (the restatements need only A @ x)."""
import numpy as np

BREAK = 2.0 ** -36   # beta_t <= BREAK * max |alpha|: the column is frozen (include/cgx.h cgx_lanczos)
EPS = 2.0 ** -52


def lanczos_f64(A, v0, steps):
    """The device's recurrence in float64 numpy, on the not yet normalised w as the kernels run it: returns (alpha, beta, m),
    alpha and beta of length `steps` with zeros at t >= m."""
    alpha, beta = np.zeros(steps), np.zeros(steps)
    w = np.array(v0, dtype=np.float64)
    u = np.zeros_like(w)
    amax, m = 0.0, steps
    ww = float(w @ w)
    for t in range(steps + 1):
        b = np.sqrt(ww)
        if t > 0:
            beta[t - 1] = b
        if t == steps:
            break
        if b <= BREAK * amax:
            m = t
            break
        y = A @ w
        a = float(w @ y) / ww
        alpha[t] = a
        amax = max(amax, abs(a))
        v = w / b
        wn = y / b - a * v - b * u
        w, u = wn, v
        ww = float(w @ w)
    return alpha, beta, m


class Lap2dOperator:
    """generate_lap2d_matrix(n) without the n x n array, for the sizes at which a dense longdouble reference costs too much: the
    non-zeros of oracle.generate_lap2d(n, row0, nrows), taken `chunk` rows at a time and kept per row, padded to the longest row
    with zeros on the row's own diagonal.  A @ x for x of shape (n,) or (n, k) in float64 or longdouble, the dtype following x
    (anything else is taken as float64); every row is summed in ascending column order.  tests/test_lap2d_operator.py compares it
    with the dense matrix."""
    __array_ufunc__ = None   # ndarray @ operator is refused, not broadcast over the object

    def __init__(self, oracle, n, chunk=1024):
        self.shape = (n, n)
        rows, cols, vals = [], [], []
        for r0 in range(0, n, chunk):
            block = oracle.generate_lap2d(n, r0, min(chunk, n - r0))
            r, c = np.nonzero(block)                          # row-major: ascending columns within a row
            rows.append(r + r0)
            cols.append(c)
            vals.append(block[r, c])
        rows, cols, vals = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
        count = np.bincount(rows, minlength=n)
        self.nnz = int(count.sum())
        first = np.concatenate([[0], np.cumsum(count)[:-1]])
        k = np.arange(self.nnz) - first[rows]                 # the entry's position in its row
        self.cols = np.repeat(np.arange(n)[:, None], int(count.max()), axis=1)
        self.vals = np.zeros(self.cols.shape)
        self.cols[rows, k] = cols
        self.vals[rows, k] = vals

    def __matmul__(self, x):
        x = np.asarray(x)
        if x.dtype != np.longdouble:
            x = x.astype(np.float64, copy=False)
        assert x.ndim in (1, 2) and x.shape[0] == self.shape[0], x.shape
        vals = self.vals.astype(x.dtype, copy=False)
        y = np.zeros(x.shape, dtype=x.dtype)
        for k in range(self.cols.shape[1]):                   # ascending position: one fixed order per row
            xk = x[self.cols[:, k]]
            y += vals[:, k] * xk if x.ndim == 1 else vals[:, k, None] * xk
        return y


def is_operator(A):
    return isinstance(A, Lap2dOperator)


def as_matrix(A, dtype):
    """np.asarray(A, dtype) for arrays; a matrix-free operator as it is (its products take the operand's dtype)."""
    return A if is_operator(A) else np.asarray(A, dtype=dtype)


def lanczos_longdouble(A, v0, steps):
    """Lanczos in longdouble with full reorthogonalisation (twice) against every earlier vector: (alpha, beta) of length steps."""
    Al = as_matrix(A, np.longdouble)
    v = np.asarray(v0, dtype=np.longdouble)
    v = v / np.sqrt(v @ v)
    V = [v]
    alpha, beta = np.zeros(steps, dtype=np.longdouble), np.zeros(steps, dtype=np.longdouble)
    b_prev, v_prev = np.longdouble(0), np.zeros_like(v)
    for t in range(steps):
        y = Al @ v
        a = v @ y
        w = y - a * v - b_prev * v_prev
        for _ in range(2):
            for q in V:
                w = w - (q @ w) * q
        b = np.sqrt(w @ w)
        alpha[t], beta[t] = a, b
        v_prev, b_prev = v, b
        v = w / b
        V.append(v)
    return alpha, beta


def jacobi_matrix(alpha, beta, m):
    T = np.diag(np.asarray(alpha[:m], dtype=np.float64))
    for i in range(m - 1):
        T[i, i + 1] = T[i + 1, i] = beta[i]
    return T


def gauss_rule(alpha, beta, m):
    """(theta ascending, weights) of the m-point rule by numpy.linalg.eigh of the dense Jacobi matrix."""
    theta, Q = np.linalg.eigh(jacobi_matrix(alpha, beta, m))
    return theta, Q[0] ** 2


def quadrature(alpha, beta, m, z2, f):
    theta, wgt = gauss_rule(alpha, beta, m)
    return float(z2 * np.sum(wgt * f(theta)))


def hash_mix64(z):
    """splitmix64's finaliser on uint64 arrays (wrapping arithmetic), as include/cgx.h states it."""
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def rademacher(seed, nprobe, n):
    """The library's probes: element i of probe j is -1 where the top bit of hash_mix64(hash_mix64(seed) ^ (j << 32 | i)) is set."""
    sm = hash_mix64(np.array([int(seed) & ((1 << 64) - 1)], dtype=np.uint64))[0]
    j = np.arange(nprobe, dtype=np.uint64)[:, None]
    i = np.arange(n, dtype=np.uint64)[None, :]
    h = hash_mix64(sm ^ ((j << np.uint64(32)) | i))
    return np.where((h >> np.uint64(63)) != 0, -1.0, 1.0)


def tolerance(d_cpu, n):
    """The rule of DESIGN.md section 17: the device may deviate from a high-precision reference by 16 x what the float64 numpy
    restatement of the same recurrence deviates (the 16 covers the device's different sum orders), with n 2^-52 as the floor."""
    return 16.0 * max(float(d_cpu), n * EPS)


def householder_matrix(n, d_values, seed):
    """A = H D H with H = I - 2 u u^T (u a seeded unit vector) and D cycling through d_values: (A, H, d).  Symmetric exactly."""
    rng = np.random.default_rng(seed)
    u = rng.standard_normal(n)
    u /= np.linalg.norm(u)
    H = np.eye(n) - 2.0 * np.outer(u, u)
    d = np.asarray(d_values, dtype=np.float64)[np.arange(n) % len(d_values)]
    A = (H * d[None, :]) @ H
    A = 0.5 * (A + A.T)
    return A, H, d
