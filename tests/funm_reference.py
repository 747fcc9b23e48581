"""Host restatements for the matrix-function tests (tests/test_funm_abi.py, tests/test_gpu_funm.py): the recurrence of
lanczos_reference.lanczos_f64 with the Lanczos vectors kept, the coefficients f(T) e_1 through numpy.linalg.eigh of the dense Jacobi
matrix, the combine, the lagged convergence indicator of cgx_apply_function, and the two references: H f(D) H b in longdouble for
lanczos_reference.householder_matrix, Q f(Theta) Q^T b from float64 eigh otherwise.  Not a test module and not part of the product."""
import numpy as np

import lanczos_reference as ref

FN_SQRT, FN_INVSQRT, FN_INV, FN_LOG, FN_EXP = 0, 1, 2, 3, 4
NAMES = {FN_SQRT: "sqrt", FN_INVSQRT: "invsqrt", FN_INV: "inv", FN_LOG: "log", FN_EXP: "exp"}


def scalar_function(fn, param=0.0):
    """f of include/cgx.h's CGX_FN_*, on arrays of any float dtype."""
    return {FN_SQRT: np.sqrt, FN_INVSQRT: lambda t: 1.0 / np.sqrt(t), FN_INV: lambda t: 1.0 / t, FN_LOG: np.log,
            FN_EXP: lambda t: np.exp(-t.dtype.type(param) * t)}[fn]


def derivative_bound(fn, param, lo, hi):
    """max |f'| over [lo, hi] (0 < lo <= hi): every f here has a monotone |f'|, so it sits at an end of the interval."""
    d = {FN_SQRT: lambda t: 0.5 / np.sqrt(t), FN_INVSQRT: lambda t: 0.5 * t ** -1.5, FN_INV: lambda t: t ** -2.0, FN_LOG: lambda t: 1.0 / t,
         FN_EXP: lambda t: param * np.exp(-param * t)}[fn]
    return float(max(d(lo), d(hi)))


def lanczos_f64_basis(A, v0, steps):
    """lanczos_reference.lanczos_f64 with the normalised v_t kept: (alpha, beta, m, V, z2), V of shape (m, n), z2 = ||v0||^2."""
    alpha, beta = np.zeros(steps), np.zeros(steps)
    w = np.array(v0, dtype=np.float64)
    u = np.zeros_like(w)
    amax, m = 0.0, steps
    ww = float(w @ w)
    z2 = ww
    V = []
    for t in range(steps + 1):
        b = np.sqrt(ww)
        if t > 0:
            beta[t - 1] = b
        if t == steps:
            break
        if b <= ref.BREAK * amax:
            m = t
            break
        y = A @ w
        a = float(w @ y) / ww
        alpha[t] = a
        amax = max(amax, abs(a))
        v = w / b
        V.append(v)
        wn = y / b - a * v - b * u
        w, u = wn, v
        ww = float(w @ w)
    alpha[m:] = 0.0
    beta[m:] = 0.0
    return alpha, beta, m, np.array(V), z2


def coefficients(alpha, beta, m, fn, param=0.0):
    """f(T_m) e_1 = Q f(Theta) Q^T e_1 by numpy.linalg.eigh of the dense Jacobi matrix."""
    theta, Q = np.linalg.eigh(ref.jacobi_matrix(alpha, beta, m))
    return Q @ (scalar_function(fn, param)(theta) * Q[0])


def change(c_m, c_lag):
    """|| c(m) - pad(c(lag)) || / || c(m) || with the sums in ascending t, as cgx_apply_function states it."""
    m, lag = len(c_m), len(c_lag)
    if lag == 0:
        return 1.0
    num = den = 0.0
    for t in range(m):
        d = float(c_m[t]) - (float(c_lag[t]) if t < lag else 0.0)
        num += d * d
        den += float(c_m[t]) * float(c_m[t])
    return 0.0 if den == 0.0 else float(np.sqrt(num) / np.sqrt(den))


def lag_of(m):
    return m - max(1, m // 8)


def combine(run, fn, param=0.0):
    """From a kept run (lanczos_f64_basis): (x, coef, change) of the device's definition, coefficients through eigh."""
    alpha, beta, m, V, z2 = run
    scale = np.sqrt(z2)
    c = scale * coefficients(alpha, beta, m, fn, param)
    lag = lag_of(m)
    c_lag = scale * coefficients(alpha, beta, lag, fn, param) if lag > 0 else np.zeros(0)
    return c @ V, c, change(c, c_lag)


def apply_f64(A, b, steps, fn, param=0.0):
    return combine(lanczos_f64_basis(A, b, steps), fn, param)


def householder_reference(H, d, b, fn, param=0.0):
    """H f(D) H b in longdouble (A = H D H with H an exact reflector in exact arithmetic)."""
    Hl, dl = np.asarray(H, dtype=np.longdouble), np.asarray(d, dtype=np.longdouble)
    return Hl @ (scalar_function(fn, param)(dl) * (Hl @ np.asarray(b, dtype=np.longdouble)))


def eigh_reference(lam, Q, b, fn, param=0.0):
    """Q f(Lambda) Q^T b from a float64 eigen-decomposition the caller made once."""
    return Q @ (scalar_function(fn, param)(lam) * (Q.T @ b))


def deviation(x, x_ref):
    x_ref = np.asarray(x_ref)
    diff = np.asarray(x, dtype=x_ref.dtype) - x_ref
    return float(np.sqrt(diff @ diff) / np.sqrt(x_ref @ x_ref))
