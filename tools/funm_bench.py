"""Matrix functions by Lanczos (cgx_apply_function): one JSON object per line.

--mode step      what keeping the basis costs per step: the wall-time difference between a --long and a --short step apply_function
                 (FN_SQRT) against the same difference for lanczos on the same context, alternated, on the symmetric dense hash matrix
                 (SPD by a dominant diagonal, filled on the device) for every N and k; medians over --repeat alternated rounds.  The
                 uploads, set-up launches and the synchronisation cancel in both; what does NOT cancel in apply_function's difference
                 is the host's coefficient work (two O(m^2) sweeps per column, the columns on host threads of their own) and the
                 longer combine launch, so the time of the same cgx_tridiag_function calls made one after the other is measured
                 beside it and reported per step and per column.
--mode combine   --repeat apply_function calls of --long steps at the first N and k, for a `rocprofv3 --kernel-trace --stats` run of
                 this program: the line carries the bytes k_funm_combine streams per launch (8 n m k).
--mode workload  one call on the kernel matrix of the tests at --workload-n (8 vectors, FN_SQRT, 256 steps): wall time (median
                 over --repeat calls behind a warm-up call), change, and the error against numpy.linalg.eigh on the host.
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


def hash_solver(pkg, n):
    s = pkg.CGSolver(gemv_variant=-1)
    s.generate_lap2d_matrix(n)
    s.probe_fill_matrix_hash(SEED, symmetric=True, diag=1.03 * 2.0 * np.sqrt(n / 3.0))
    return s


def lag_of(m):
    return m - max(1, m // 8)


def mode_step(pkg, a):
    cgx = pkg.cgx
    for n in a.ns:
        with hash_solver(pkg, n) as s:
            rng = np.random.default_rng(n)
            for k in a.ks:
                V = rng.standard_normal((k, n))

                def lanczos(steps):
                    return wall(lambda: s.lanczos(V, steps))

                def apply(steps):
                    return wall(lambda: s.apply_function(V, cgx.FN_SQRT, steps))

                def host(alpha, beta, steps):                 # the coefficient work of one call, on the host alone
                    def run():
                        for j in range(k):
                            cgx.tridiag_function(alpha[j, :steps], beta[j, :steps], cgx.FN_SQRT)
                            cgx.tridiag_function(alpha[j, :lag_of(steps)], beta[j, :lag_of(steps)], cgx.FN_SQRT)
                    return wall(run)

                alpha, beta, _ = s.lanczos(V, a.long)
                apply(a.long)                                 # warm: the basis block is made at its largest size
                apply(a.short)
                lz, ap, ho = [], [], []
                for _ in range(a.repeat):
                    lz.append((lanczos(a.long) - lanczos(a.short)) / (a.long - a.short))
                    ap.append((apply(a.long) - apply(a.short)) / (a.long - a.short))
                    ho.append((host(alpha, beta, a.long) - host(alpha, beta, a.short)) / (a.long - a.short))
                ms_l, ms_a, ms_h = (1e3 * statistics.median(v) for v in (lz, ap, ho))
                emit({"mode": "step", "n": n, "k": k, "lanczos_ms_per_step": ms_l, "apply_ms_per_step": ms_a,
                      "overhead_us_per_step": 1e3 * (ms_a - ms_l), "host_coefficients_us_per_step_per_column": 1e3 * ms_h / k,
                      "overhead_fraction": ms_a / ms_l - 1.0, "copy_bytes_per_step": 16 * n * k, "A_bytes_per_step": 8 * n * n,
                      "short": a.short, "long": a.long, "repeat": a.repeat}, a.out)


def mode_combine(pkg, a):
    cgx = pkg.cgx
    n, k = a.ns[0], a.ks[0]
    with hash_solver(pkg, n) as s:
        V = np.random.default_rng(n).standard_normal((k, n))
        for _ in range(a.repeat):
            _, info = s.apply_function(V, cgx.FN_SQRT, a.long)
    emit({"mode": "combine", "n": n, "k": k, "steps": a.long, "launches": a.repeat, "steps_done": [int(m) for m in info["steps_done"]],
          "basis_bytes_per_launch": 8 * n * int(np.sum(info["steps_done"]))}, a.out)


def mode_workload(pkg, a):
    cgx = pkg.cgx
    n, k, steps = a.workload_n, 8, 256
    A = kernel_matrix(n)
    B = np.random.default_rng(20261020).standard_normal((k, n))
    t0 = time.perf_counter()
    lam, Q = np.linalg.eigh(A)
    t_host = time.perf_counter() - t0
    X_ref = ((B @ Q) * np.sqrt(lam)[None, :]) @ Q.T
    with pkg.CGSolver(gemv_variant=-1) as s:
        s.set_matrix_dense(A)
        X, info = s.apply_function(B, cgx.FN_SQRT, steps)
        times = [wall(lambda: s.apply_function(B, cgx.FN_SQRT, steps)) for _ in range(a.repeat)]
    err = [float(np.linalg.norm(X[j] - X_ref[j]) / np.linalg.norm(X_ref[j])) for j in range(k)]
    emit({"mode": "workload", "n": n, "k": k, "fn": "sqrt", "steps": steps, "apply_s": statistics.median(times),
          "steps_done": [int(m) for m in info["steps_done"]], "change": [float(c) for c in info["change"]], "error_vs_eigh": err,
          "condition_number": float(lam[-1] / lam[0]), "numpy_eigh_host_s": t_host, "repeat": a.repeat}, a.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["step", "combine", "workload"], required=True)
    ap.add_argument("--ns", type=int, nargs="+", default=[4096, 10000, 32768])
    ap.add_argument("--ks", type=int, nargs="+", default=[8, 16])
    ap.add_argument("--short", type=int, default=20)
    ap.add_argument("--long", type=int, default=120)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--workload-n", type=int, default=4096)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch  # noqa: F401  (first: libcgx then binds to the HIP runtime torch loaded)
    import __graft_entry__ as g
    pkg = g.load_package()
    {"step": mode_step, "combine": mode_combine, "workload": mode_workload}[a.mode](pkg, a)


if __name__ == "__main__":
    main()
