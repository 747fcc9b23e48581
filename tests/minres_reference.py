"""Host reference of cgx_solve_minres (pinned by tests/test_minres_abi.py, judges tests/test_gpu_minres.py):
Paige-Saunders MINRES for (A + sigma_j I) x_j = b on ONE Lanczos recurrence from r0 = b, in plain numpy, in np.float64 or
np.longdouble, with the library's breakdown and singular rules and its iteration numbering.  No scipy.

    beta_0 = ||b||, v_0 = b / beta_0, v_-1 = 0
    step t:   y = A v_t;  alpha_t = v_t . y;  w = y - alpha_t v_t - beta_t v_(t-1);  beta_(t+1) = ||w||
    column t of T + sigma I, (beta_t, alpha_t + sigma, beta_(t+1)), reduced by the two previous rotations and a new one (c, s) to
    (eps, delta, gamma);  d_t = (v_t - delta d_(t-1) - eps d_(t-2)) / gamma;  x += c phibar d_t;  phibar <- s phibar

Iteration t (0-based) applies column t.  A shift is frozen in iteration t with converged = 1 when |phibar_(t+1)| < tol.  A breakdown
(beta_(t+1) <= 2^-36 max_(s<=t) |alpha_s|) closes column t with beta_(t+1) := 0 and ends the recurrence: a running shift whose
diagonal entry in front of the last rotation is <= 2^-36 (max |alpha| + |sigma|) keeps its x and reports converged = 0, every other
one takes the column and reports converged = 1, residual_last = 0; both with iterations = t.  A rotation or step length that is not
finite freezes the shift unconverged.  Shifts still running after max_iter columns report converged = 0, iterations = max_iter."""
import numpy as np

import long_vector_reference as lv

BREAK = 2.0 ** -36

# The 16 shifts of the long-vector run (tests/test_gpu_minres_edges.py; lap2d, b = long_vector_reference.normal_b, 12 columns at
# tol 1e-6): 100, -20, -1e4, 30, 1e3, 200, -50 and 3e4 freeze on the way, the others run out.  tests/test_minres_abi.py pins that
# no shift's residual_last lies in [0.7 tol, 1.5 tol] and no residual_prev of a frozen one below 1.05 tol.
LONG_SHIFTS = [0.0, 1.0, -1.0, 100.0, -3.7, -20.0, -1e4, 30.0, 1e3, 0.5, -0.25, 200.0, -50.0, 2.5, 3e4, -6.0]
LONG_TOL = 1e-6


def tile_shifts(n):
    """The shifts of the symmetric hash matrix with a zero diagonal at the sizes past 256 K1 partials: its spectral radius is about
    r = 2 sqrt(n / 3), so +-r/2 lie inside the spectrum, +-3r/2 and 1e4 outside, and no eigenvalue has to be computed."""
    r = 2.0 * np.sqrt(n / 3.0)
    return [0.0, 1.0, -1.0, 0.5 * r, -0.5 * r, 1.5 * r, -1.5 * r, 1e4]


def operator(A, dtype):
    """x -> A x for a dense array, a CSR triple (indptr, indices, data) or a callable (taken as it is)."""
    if callable(A):
        return A
    if isinstance(A, tuple):
        indptr, indices, data = A
        data = np.asarray(data).astype(dtype)
        return lambda x: lv.matvec(indptr, indices, data, x)
    Ad = np.asarray(A).astype(dtype, copy=False)
    return lambda x: Ad @ x


def minres(A, b, sigmas, max_iter, tol=0.0, dtype=np.float64):
    """Returns one dict per shift: x (fp64), iterations, converged, residual_prev, residual_last (|phibar| in front of and behind
    the shift's last column)."""
    mv = operator(A, dtype)
    b = np.asarray(b).astype(dtype)
    n = b.size
    zero, brk = dtype(0), dtype(BREAK)
    beta0 = np.sqrt(b @ b)
    sh = [dict(sigma=dtype(s), cs=dtype(-1), sn=zero, dbar=zero, eps=zero, phibar=beta0, d1=np.zeros(n, dtype), d2=np.zeros(n, dtype),
               x=np.zeros(n, dtype), running=True, iterations=max_iter, converged=0, residual_prev=beta0, residual_last=beta0)
          for s in sigmas]

    def freeze(q, t, converged):
        q.update(running=False, iterations=t, converged=converged)

    if not (beta0 > 0 and np.isfinite(beta0)):      # b = 0: x = 0 solves every system
        for q in sh:
            freeze(q, 0, 1 if beta0 == 0 else 0)
        max_iter = 0
    else:
        v, vprev, beta, amax = b / beta0, np.zeros(n, dtype), beta0, zero
    for t in range(max_iter):
        y = mv(v)
        alpha = v @ y
        w = y - alpha * v - beta * vprev
        bnext = np.sqrt(w @ w)
        amax = max(amax, abs(alpha))
        breakdown = bool(bnext <= brk * amax)
        bn = zero if breakdown else bnext
        for q in sh:
            if not q["running"]:
                continue
            alfa = alpha + q["sigma"]
            delta = q["cs"] * q["dbar"] + q["sn"] * alfa
            gbar = q["sn"] * q["dbar"] - q["cs"] * alfa
            eps_old = q["eps"]
            q["eps"], q["dbar"] = q["sn"] * bn, -q["cs"] * bn
            with np.errstate(over="ignore"):        # |sigma| of 1e155 and more: gamma = inf, and the shift freezes below
                gamma = np.sqrt(gbar * gbar + bn * bn)
            if breakdown and abs(gbar) <= brk * (amax + abs(q["sigma"])):   # singular on the Krylov space: x stays
                q["residual_prev"] = q["residual_last"] = abs(q["phibar"])
                freeze(q, t, 0)
                continue
            with np.errstate(all="ignore"):
                c, s = gbar / gamma, bn / gamma
                phi, phibar_new = c * q["phibar"], s * q["phibar"]
            if not (np.isfinite(gamma) and np.isfinite(phi)):
                q["residual_prev"] = q["residual_last"] = abs(q["phibar"])
                freeze(q, t, 0)
                continue
            d = (v - delta * q["d1"] - eps_old * q["d2"]) / gamma
            q["x"] += phi * d
            q["d2"], q["d1"] = q["d1"], d
            q["residual_prev"], q["residual_last"] = abs(q["phibar"]), (zero if breakdown else abs(phibar_new))
            q["cs"], q["sn"], q["phibar"] = c, s, phibar_new
            if breakdown or q["residual_last"] < tol:
                freeze(q, t, 1)
        if breakdown or not any(q["running"] for q in sh):
            break
        vprev, v, beta = v, w / bnext, bnext
    return [dict(x=q["x"].astype(np.float64), iterations=int(q["iterations"]), converged=int(q["converged"]),
                 residual_prev=float(q["residual_prev"]), residual_last=float(q["residual_last"])) for q in sh]
