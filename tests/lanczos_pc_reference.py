"""Host restatements for the preconditioned Lanczos quadrature tests (tests/test_lanczos_pc_abi.py, tests/test_gpu_lanczos_pc.py;
DESIGN.md section 18): the recurrence of csrc/cgx_lanczos_pc.hip in float64 numpy on the unnormalised u as the kernels run it, a
longdouble version with full reorthogonalisation (twice) in the M-inner product, the library's probes of covariance M, the
preconditioners as closures, and the matrix of the breakdown test.  Not a test module and not part of the product."""
import numpy as np

import lanczos_reference as ref
import pivchol_reference as pref

LD = np.longdouble
BREAK = ref.BREAK


def jacobi_apply(A, dtype=np.float64):
    """u = D^-1 w.  float64: through the rounded inverse diagonal, as the device multiplies; longdouble: the division."""
    d = np.diag(np.asarray(A)).astype(dtype)
    if dtype is np.float64:
        dinv = 1.0 / d
        return lambda w: dinv * w
    return lambda w: np.asarray(w).astype(dtype) / d


def lowrank_apply(L, delta, dtype=np.float64):
    """u = (L L^T + delta I)^-1 w by the Woodbury identity, from the device's own L and delta.  float64: as the kernels run it,
    u = (w - L (C^-1 (L^T w))) / delta with C = delta I + L^T L inverted ONCE, explicitly, by the set-up's symmetric sweep without
    pivoting (sweep_inverse), whose error -- not that of the recurrence -- sets the level of the quadratures' deviations;
    longdouble: the Cholesky solve of pivchol_reference."""
    if dtype is not np.float64:
        return pref.Woodbury(L, delta, dtype).apply
    L = np.asarray(L, dtype=np.float64)
    Cinv = sweep_inverse(L.T @ L + delta * np.eye(L.shape[1]))
    return lambda w: (w - L @ (Cinv @ (L.T @ w))) / delta


def sweep_inverse(C):
    """The set-up's inversion of an SPD block (k_bj_invert, csrc/cgx_kernels.hip) in float64 numpy: for k = 0 ... m-1, with c =
    column k of the current matrix and d = 1 / c_k: a_kk = -d, a_ik = a_ki = c_i d, a_ij -= (c_i d) c_j elsewhere; then -a."""
    a = np.array(C, dtype=np.float64)
    m = a.shape[0]
    for k in range(m):
        c = a[:, k].copy()
        d = 1.0 / c[k]
        f = c * d
        a -= np.outer(f, c)
        a[:, k] = f
        a[k, :] = f
        a[k, k] = -d
    return -0.5 * (a + a.T)


def lanczos_pc_f64(A, apply, v0, steps):
    """The device's recurrence in float64 numpy: returns (alpha, beta, m, eta2), alpha and beta of length `steps` with zeros at
    t >= m.  w lives on the side of M, u = M^-1 w; the mat-vec runs on the not yet normalised u and the step divides by beta."""
    alpha, beta = np.zeros(steps), np.zeros(steps)
    w = np.array(v0, dtype=np.float64)
    u = apply(w)
    vprev = np.zeros_like(w)
    ww = float(w @ u)
    eta2 = ww
    assert ww > 0.0 and np.isfinite(ww), ww
    amax, m = 0.0, steps
    for t in range(steps + 1):
        b = np.sqrt(ww) if ww > 0.0 else 0.0
        if t > 0:
            beta[t - 1] = b
        if t == steps:
            break
        if not ww > 0.0 or b <= BREAK * amax:
            m = t
            break
        y = A @ u
        a = float(u @ y) / ww
        alpha[t] = a
        amax = max(amax, abs(a))
        v = w / b
        wn = y / b - a * v - b * vprev
        w, vprev = wn, v
        u = apply(w)
        ww = float(w @ u)
    alpha[m:] = 0.0
    beta[m:] = 0.0
    return alpha, beta, m, eta2


def lanczos_pc_longdouble(A, apply_ld, v0, steps):
    """The same recurrence in longdouble with full reorthogonalisation, twice per step, in the M^-1 inner product of the w side:
    the coefficient of v_s in w is v_s^T M^-1 w = q_s . w with q_s = M^-1 v_s.  Returns (alpha, beta, eta2)."""
    Al = np.asarray(A, dtype=LD)
    w = np.asarray(v0, dtype=LD)
    u = apply_ld(w)
    eta2 = w @ u
    b = np.sqrt(eta2)
    V, Q = [], []
    alpha, beta = np.zeros(steps, dtype=LD), np.zeros(steps, dtype=LD)
    v_prev, b_prev = np.zeros_like(w), LD(0)
    for t in range(steps):
        v, q = w / b, u / b
        V.append(v)
        Q.append(q)
        y = Al @ q
        a = q @ y
        w = y - a * v - b_prev * v_prev
        for _ in range(2):
            for vs, qs in zip(V, Q):
                w = w - (qs @ w) * vs
        u = apply_ld(w)
        b_prev, v_prev = b, v
        b = np.sqrt(w @ u)
        alpha[t], beta[t] = a, b
    return alpha, beta, eta2


def probes_log_jacobi(seed, nprobe, A):
    """cgx_slq_probes(CGX_SLQ_LOG) under point Jacobi: z_i = s_i sqrt(A_ii)."""
    n = A.shape[0]
    return ref.rademacher(seed, nprobe, n) * np.sqrt(np.diag(A))[None, :]


def probes_log_lowrank(seed, nprobe, L, delta):
    """cgx_slq_probes(CGX_SLQ_LOG) under the pivoted-Cholesky factor: z = L g + sqrt(delta) s, s the signs of elements 0 .. n-1 and
    g those of elements n .. n + rank - 1 of the same probe; per row one chain over the columns in ascending order from +0.0 (the
    products with +-1 are exact, so the device's fma chain rounds as this sum does)."""
    n, k = L.shape
    S = ref.rademacher(seed, nprobe, n + k)
    Z = np.zeros((nprobe, n))
    for t in range(k):
        Z = Z + L[None, :, t] * S[:, n + t, None]
    return Z + np.sqrt(delta) * S[:, :n]


def breakdown_matrix(n=1000, seed=20261020):
    """A = S B S with s log-uniform in [1, 100] and B = I + (3 1 1^T + 7 v2 v2^T + 0.5 v3 v3^T) / n, v2 = (+,-,+,-,...), v3 =
    (+,+,-,-,...) (n a multiple of 4: the three vectors are orthogonal).  B's diagonal is constant, so D^-1/2 A D^-1/2 = B / B_00
    has the four eigenvalues (1 + c) / B_00, c = 0, 3, 7, 0.5.  Returns (A, s, vectors (3, n), c (3,), B_00)."""
    assert n % 4 == 0
    s = np.exp(np.random.default_rng(seed).uniform(0.0, np.log(100.0), n))
    i = np.arange(n)
    vec = np.array([np.ones(n), np.where(i % 2 == 0, 1.0, -1.0), np.where(i % 4 < 2, 1.0, -1.0)])
    c = np.array([3.0, 7.0, 0.5])
    B = np.eye(n) + (vec.T * c[None, :]) @ vec / n
    A = (s[:, None] * B) * s[None, :]
    A = 0.5 * (A + A.T)
    return A, s, vec, c, 1.0 + float(c.sum()) / n


def breakdown_log_quadratic(g, vec, c, b00=None):
    """g^T log(B / B_00) g in longdouble from the spectral form of B: log(B / B_00) = -log(B_00) I + sum_k log(1 + c_k) v_k v_k^T / n
    (b00 None: the exact 1 + sum(c) / n)."""
    g = np.asarray(g, dtype=LD)
    n = LD(len(g))
    return breakdown_log_terms(g, vec, c, b00).sum()


def breakdown_log_terms(g, vec, c, b00=None):
    """The four terms of breakdown_log_quadratic (their sum of moduli is the scale a relative tolerance refers to: the terms cancel)."""
    g = np.asarray(g, dtype=LD)
    n = LD(len(g))
    b00 = LD(1) + np.sum(np.asarray(c, dtype=LD)) / n if b00 is None else LD(b00)
    return np.array([-np.log(b00) * (g @ g)] + [np.log(LD(1) + LD(c[k])) * (vec[k].astype(LD) @ g) ** 2 / n for k in range(len(c))])
