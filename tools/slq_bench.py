"""Lanczos quadrature (cgx_lanczos / cgx_trace_slq): one JSON object per line.

--mode step    the time of one Lanczos step (the plain K1m + k_lanczos_step) against one cgx_solve_multi iteration (the fused K1m +
               k_multi_update) at the same k on the same context, alternated, on the symmetric dense hash matrix (SPD by a dominant
               diagonal, filled on the device) for every N and k.  Both are wall-time differences between a long and a short call
               (--long / --short steps or iterations at tol = 0), so the uploads, downloads and set-up launches cancel; medians over
               --repeat alternated rounds.
--mode logdet  the wall time of one logdet call (16 probes, 100 steps) on the kernel matrix of the tests at n = 4096, median over
               --repeat calls behind a warm-up call, and for orientation the host time of numpy.linalg.slogdet on the same matrix.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SEED = 0x3D1F


def kernel_matrix(n, ell=0.2, sigma2=1e-2, seed=20261018):
    """A = S K S + sigma^2 I with a Gaussian kernel on uniform points of the unit square, s log-uniform in [1, 4]."""
    rng = np.random.default_rng(seed)
    pts = rng.random((n, 2))
    s = np.exp(rng.uniform(0.0, np.log(4.0), n))
    d2 = ((pts[:, None, :] - pts[None, :, :]) ** 2).sum(axis=2)
    A = s[:, None] * np.exp(-d2 / (2.0 * ell * ell)) * s[None, :]
    A = 0.5 * (A + A.T)
    A[np.diag_indices(n)] += sigma2
    return A


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def wall(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def mode_step(pkg, a):
    for n in a.ns:
        with pkg.CGSolver(gemv_variant=-1) as s:
            s.generate_lap2d_matrix(n)
            s.probe_fill_matrix_hash(SEED, symmetric=True, diag=1.03 * 2.0 * np.sqrt(n / 3.0))
            s.tolerance(0.0)
            rng = np.random.default_rng(n)
            for k in a.ks:
                V = rng.standard_normal((k, n))

                def multi(iters):
                    s.set_max_iter(iters)
                    return wall(lambda: s.solve_multi(V))

                def lanczos(steps):
                    return wall(lambda: s.lanczos(V, steps))

                multi(a.short)
                lanczos(a.short)
                lz, mu = [], []
                for _ in range(a.repeat):
                    lz.append((lanczos(a.long) - lanczos(a.short)) / (a.long - a.short))
                    mu.append((multi(a.long) - multi(a.short)) / (a.long - a.short))
                ms_l, ms_m = 1e3 * statistics.median(lz), 1e3 * statistics.median(mu)
                emit({"mode": "step", "n": n, "k": k, "lanczos_ms_per_step": ms_l, "multi_ms_per_iteration": ms_m,
                      "ratio": ms_l / ms_m, "A_GBps_lanczos": 8.0 * n * n / (ms_l * 1e-3) / 1e9, "short": a.short, "long": a.long,
                      "repeat": a.repeat}, a.out)


def mode_logdet(pkg, a):
    n, probes, steps = a.logdet_n, 16, 100
    A = kernel_matrix(n)
    t0 = time.perf_counter()
    sign, exact = np.linalg.slogdet(A)
    t_host = time.perf_counter() - t0
    with pkg.CGSolver(gemv_variant=-1) as s:
        s.set_matrix_dense(A)
        out = s.logdet(probes=probes, steps=steps)
        times = [wall(lambda: s.logdet(probes=probes, steps=steps)) for _ in range(a.repeat)]
    emit({"mode": "logdet", "n": n, "probes": probes, "steps": steps, "logdet_s": statistics.median(times), "estimate": out["estimate"],
          "std_error": out["std_error"], "ritz_min": out["ritz_min"], "ritz_max": out["ritz_max"], "numpy_slogdet": float(exact),
          "numpy_slogdet_host_s": t_host, "repeat": a.repeat}, a.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["step", "logdet"], required=True)
    ap.add_argument("--ns", type=int, nargs="+", default=[4096, 10000, 32768])
    ap.add_argument("--ks", type=int, nargs="+", default=[8, 16])
    ap.add_argument("--short", type=int, default=20)
    ap.add_argument("--long", type=int, default=120)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--logdet-n", type=int, default=4096)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch  # noqa: F401  (first: libcgx then binds to the HIP runtime torch loaded)
    import __graft_entry__ as g
    pkg = g.load_package()
    (mode_step if a.mode == "step" else mode_logdet)(pkg, a)


if __name__ == "__main__":
    main()
