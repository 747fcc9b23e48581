"""Host restatement for the eigenpair tests (tests/test_eigs_abi.py, tests/test_gpu_eigs.py): the recurrence of cgx_eigenpairs
(include/cgx.h, csrc/cgx_eigs.hip) in float64 numpy -- Lanczos with classical Gram-Schmidt against the whole
basis, run twice per step -- with the Ritz pairs through numpy.linalg.eigh of the dense Jacobi matrix and the tol rule of the
library, and the test matrices the two files share."""
import numpy as np

import lanczos_reference as ref

LARGEST, SMALLEST = 0, 1   # CGX_EIG_*
POLL = 16                  # tol > 0: the Ritz estimates are looked at behind every step with (t + 1) % POLL == 0, and the last


def lanczos_reorth_f64(A, v0, steps):
    """(alpha, beta, m, Q): alpha, beta of length `steps` with zeros at t >= m; Q has steps + 1 rows: q_0 .. q_(m-1) and, when the
    run was not frozen, q_m; the rows behind them are zero."""
    A = ref.as_matrix(A, np.float64)                         # an array as before; a matrix-free operator as it is
    n = A.shape[0]
    alpha, beta = np.zeros(steps), np.zeros(steps)
    v0 = np.asarray(v0, dtype=np.float64)
    Q = np.zeros((steps + 1, n))
    Q[0] = v0 / np.sqrt(float(v0 @ v0))
    amax, m, b_prev = 0.0, steps, 0.0
    for t in range(steps):
        q = Q[t]
        y = A @ q
        a = float(q @ y)
        alpha[t] = a
        amax = max(amax, abs(a))
        w = y - a * q
        if t > 0:
            w = w - b_prev * Q[t - 1]
        for _ in range(2):                                   # classical Gram-Schmidt, twice: h from the w the pass began with
            h = Q[:t + 1] @ w
            w = w - h @ Q[:t + 1]
        b = float(np.sqrt(w @ w))
        beta[t] = b
        if b <= ref.BREAK * amax:                            # an invariant subspace: frozen with m = t + 1
            m = t + 1
            break
        Q[t + 1] = w / b
        b_prev = b
    return alpha, beta, m, Q


def ritz(alpha, beta, m, which, nev):
    """The wanted Ritz pairs of the leading m x m block: (values, S, estimates, scale, theta) -- values descending for LARGEST,
    ascending for SMALLEST; S[j] the unit eigenvector of T with S[j, 0] >= 0; estimates[j] = beta_(m-1) |S[j, m-1]|; scale = max
    |theta| over all Ritz values; nfound = min(nev, m) entries."""
    theta, V = np.linalg.eigh(ref.jacobi_matrix(alpha, beta, m))
    nf = min(nev, m)
    idx = [m - 1 - j for j in range(nf)] if which == LARGEST else list(range(nf))
    S = V[:, idx].T.copy()
    S[S[:, 0] < 0.0] *= -1.0
    est = beta[m - 1] * np.abs(S[:, m - 1])
    return theta[idx], S, est, float(np.max(np.abs(theta))), theta


def eigenpairs_f64(A, v0, which, nev, steps, tol=0.0, run=None):
    """cgx_eigenpairs restated: (values, vectors, info) with info = dict(residual, estimate, steps_done, nfound, alpha, beta).
    run: a kept lanczos_reorth_f64(A, v0, steps) result (the prefix property makes a shorter run its leading part)."""
    A = ref.as_matrix(A, np.float64)                         # an array as before; a matrix-free operator as it is
    n = A.shape[0]
    alpha, beta, m_full, Q = run if run is not None else lanczos_reorth_f64(A, v0, steps)
    m = m_full
    if tol > 0.0:
        t = 0
        while t < steps:
            t = min(steps, (t // POLL + 1) * POLL)
            m = min(t, m_full)
            if m < t:
                break
            _, _, est, scale, _ = ritz(alpha, beta, m, which, nev)
            if len(est) == nev and np.all(est <= tol * scale):
                break
    vals, S, est, scale, _ = ritz(alpha, beta, m, which, nev)
    nf = len(vals)
    X = S @ Q[:m]
    res = np.array([np.linalg.norm(A @ X[j] - vals[j] * X[j]) for j in range(nf)])
    pad = nev - nf
    return (np.concatenate([vals, np.zeros(pad)]), np.vstack([X, np.zeros((pad, n))]),
            {"residual": np.concatenate([res, np.zeros(pad)]), "estimate": np.concatenate([est, np.zeros(pad)]), "steps_done": m,
             "nfound": nf, "alpha": alpha, "beta": beta})


def align(X, X_ref):
    """Rows of X with the sign that brings each closest to the row of X_ref (an eigenvector is defined up to its sign)."""
    X, X_ref = np.atleast_2d(X), np.atleast_2d(X_ref)
    sign = np.where(np.sum(X * X_ref, axis=1) < 0.0, -1.0, 1.0)
    return X * sign[:, None]


def wanted(lam, Qeig, which, nev):
    """From numpy.linalg.eigh's (lam ascending, eigenvectors as columns): the nev wanted values and their vectors as rows."""
    n = len(lam)
    idx = [n - 1 - j for j in range(nev)] if which == LARGEST else list(range(nev))
    return lam[idx], Qeig[:, idx].T


def outlier_matrix(n=257, seed=5):
    """A = Q diag(lam) Q^T: lam = linspace(1, 2, n - 8) and the outliers 3, 4, 5, 6.5, 8, 10, 13, 17.  Returns (A, lam ascending)."""
    out = np.array([3.0, 4.0, 5.0, 6.5, 8.0, 10.0, 13.0, 17.0])
    lam = np.concatenate([np.linspace(1.0, 2.0, n - len(out)), out])
    Qm, _ = np.linalg.qr(np.random.default_rng(seed).standard_normal((n, n)))
    A = (Qm * lam[None, :]) @ Qm.T
    return 0.5 * (A + A.T), lam
