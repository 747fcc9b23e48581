"""Host references for the block-Jacobi tests (tests/test_gpu_block_jacobi.py): the library's PCG recurrence
 with z = D_b^-1 r restated in numpy, in np.longdouble or fp64, with the block inverses formed in the same
precision by Gauss-Jordan without pivoting; and the test matrices that are not the generator's."""
import numpy as np


def block_ranges(n, block):
    return [(s, min(s + block, n)) for s in range(0, n, block)]


def invert_spd(D, dtype=np.longdouble):
    """D^-1 of one SPD block by Gauss-Jordan without pivoting, in `dtype`."""
    m = D.shape[0]
    a = np.array(D, dtype=dtype)
    inv = np.eye(m, dtype=dtype)
    for k in range(m):
        p = a[k, k]
        a[k] /= p
        inv[k] /= p
        f = a[:, k].copy()
        f[k] = 0
        a -= np.outer(f, a[k])
        inv -= np.outer(f, inv[k])
    return inv


def block_inverses(A, block, dtype=np.longdouble):
    return [invert_spd(A[s:e, s:e], dtype) for s, e in block_ranges(A.shape[0], block)]


def apply_blocks(inv, block, r):
    z = np.empty_like(r)
    for j, w in enumerate(inv):
        s = j * block
        z[s:s + w.shape[0]] = w @ r[s:s + w.shape[0]]
    return z


def pcg(A, b, block, iters, tol=0.0, dtype=np.longdouble, keep=()):
    """The library's recurrence with z = D_b^-1 r.  Returns a dict: x (fp64), iterations as the library counts them, converged,
    residual_prev / residual_last (sqrt(r.r) before / after the last update), and xs[k] = x after k iterations for k in keep."""
    A = np.asarray(A).astype(dtype)
    b = np.asarray(b).astype(dtype)
    inv = block_inverses(A, block, dtype)
    x = np.zeros_like(b)
    r = b.copy()
    z = apply_blocks(inv, block, r)
    p = z.copy()
    rho = r @ z
    prev = np.sqrt(r @ r)
    out = {"xs": {}, "converged": 0, "iterations": iters}
    last = prev
    for k in range(iters):
        Ap = A @ p
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
        z = apply_blocks(inv, block, r)
        rn = r @ z
        p = z + (rn / rho) * p
        rho = rn
    out.update(x=x.astype(np.float64), residual_prev=float(prev), residual_last=float(last))
    return out


def four_dof_matrix(lap2d_256, seed=20261017):
    """256 nodes with 4 unknowns each: A = S (L (x) I_4) S^T, symmetrised, S block diagonal with the Cholesky factors of
    (M M^T + 0.1 I) 10^u per node (M standard normal, u uniform in [0, 2]): ill-scaled 4 x 4 node blocks.  Returns (A, b), b
    standard normal."""
    nn, m = 256, 4
    assert lap2d_256.shape == (nn, nn)
    rng = np.random.default_rng(seed)
    n = nn * m
    S = np.zeros((n, n))
    for j in range(nn):
        M = rng.standard_normal((m, m))
        u = rng.uniform(0.0, 2.0)
        S[j * m:(j + 1) * m, j * m:(j + 1) * m] = np.linalg.cholesky((M @ M.T + 0.1 * np.eye(m)) * 10.0 ** u)
    A = S @ np.kron(lap2d_256, np.eye(m)) @ S.T
    A = 0.5 * (A + A.T)
    b = rng.standard_normal(n)
    return A, b


def block_diagonal_matrix(n, block, seed):
    """Blocks M M^T + m I (m = the block's size, M standard normal) on the ranges block Jacobi uses: D_b = A."""
    rng = np.random.default_rng(seed)
    A = np.zeros((n, n))
    for s, e in block_ranges(n, block):
        m = e - s
        M = rng.standard_normal((m, m))
        A[s:e, s:e] = M @ M.T + m * np.eye(m)
    A = 0.5 * (A + A.T)
    return A, rng.standard_normal(n)
