"""Preconditioned Lanczos quadrature (cgx_lanczos_pc / cgx_trace_slq_pc): one JSON object per line.

--mode step    the time of one preconditioned Lanczos step (the plain K1m + the step launch(es) of cgx_lanczos_pc.hip) against one
               plain cgx_lanczos step and one cgx_solve_multi_pc iteration at the same k on the same context, alternated, on the
               symmetric dense hash matrix (SPD by a dominant diagonal, filled on the device) for every N, k and preconditioner
               (--ranks: pivoted-Cholesky ranks; 0 = point Jacobi).  All three are wall-time differences between a long and a short
               call (--long / --short steps or iterations at tol = 0), so the uploads, downloads and set-up launches cancel; medians
               over --repeat alternated rounds.
--mode logdet  on the kernel matrix of the tests at n = 4096 with a rank-64 factor and 16 probes: the smallest step count, in
               multiples of 4, beyond which the estimate moves by less than 0.1 standard errors; the wall time of logdet_pc at that
               count with the factor already made, and with its set-up included (the rank is changed and changed back in front of the
               call, which drops the factor); and, in the same session, logdet(16, 100) with the preconditioner off.  Medians over
               --repeat calls behind a warm-up call.
"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from slq_bench import SEED, emit, kernel_matrix, wall  # noqa: E402


def mode_step(pkg, a):
    for n in a.ns:
        with pkg.CGSolver(gemv_variant=-1) as s:
            s.generate_lap2d_matrix(n)
            s.probe_fill_matrix_hash(SEED, symmetric=True, diag=1.03 * 2.0 * np.sqrt(n / 3.0))
            s.tolerance(0.0)
            rng = np.random.default_rng(n)
            for k in a.ks:
                V = rng.standard_normal((k, n))
                for rank in a.ranks:
                    def precond():
                        s.set_preconditioner("pivchol", rank=rank) if rank else s.set_preconditioner("jacobi")

                    def multi(iters):
                        precond()
                        s.set_max_iter(iters)
                        return wall(lambda: s.solve_multi_pc(V))

                    def lanczos_pc(steps):
                        precond()
                        return wall(lambda: s.lanczos_pc(V, steps))

                    def lanczos(steps):
                        s.set_preconditioner(None)
                        return wall(lambda: s.lanczos(V, steps))

                    multi(a.short)
                    lanczos_pc(a.short)
                    lanczos(a.short)
                    lp, lz, mu = [], [], []
                    for _ in range(a.repeat):
                        lp.append((lanczos_pc(a.long) - lanczos_pc(a.short)) / (a.long - a.short))
                        lz.append((lanczos(a.long) - lanczos(a.short)) / (a.long - a.short))
                        mu.append((multi(a.long) - multi(a.short)) / (a.long - a.short))
                    ms_p, ms_l, ms_m = (1e3 * statistics.median(x) for x in (lp, lz, mu))
                    emit({"mode": "step", "n": n, "k": k, "precond": "pivchol" if rank else "jacobi", "rank": rank,
                          "lanczos_pc_ms_per_step": ms_p, "lanczos_ms_per_step": ms_l, "multi_pc_ms_per_iteration": ms_m,
                          "ratio_to_plain_step": ms_p / ms_l, "ratio_to_multi_pc_iteration": ms_p / ms_m,
                          "extra_us_over_plain_step": 1e3 * (ms_p - ms_l), "short": a.short, "long": a.long, "repeat": a.repeat}, a.out)


def mode_logdet(pkg, a):
    n, probes, rank = a.logdet_n, 16, 64
    A = kernel_matrix(n)
    sign, exact = np.linalg.slogdet(A)
    with pkg.CGSolver(gemv_variant=-1) as s:
        s.set_matrix_dense(A)
        s.set_preconditioner("pivchol", rank=rank)
        prev, steps, scan = None, 0, []
        for m in range(4, 101, 4):
            out = s.logdet_pc(probes=probes, steps=m)
            scan.append((m, out["estimate"], out["std_error"]))
            if prev is not None and abs(out["estimate"] - prev["estimate"]) < 0.1 * out["std_error"]:
                steps = m - 4                                 # beyond this count the estimate no longer moves
                break
            prev = out
        out = s.logdet_pc(probes=probes, steps=steps)
        warm = [wall(lambda: s.logdet_pc(probes=probes, steps=steps)) for _ in range(a.repeat)]

        def with_setup():
            s.set_preconditioner("pivchol", rank=rank - 1)
            s.set_preconditioner("pivchol", rank=rank)        # a new rank drops the factor: the call makes it again
            return wall(lambda: s.logdet_pc(probes=probes, steps=steps))

        with_setup()
        cold = [with_setup() for _ in range(a.repeat)]
        s.set_preconditioner(None)
        plain = s.logdet(probes=probes, steps=100)
        t_plain = [wall(lambda: s.logdet(probes=probes, steps=100)) for _ in range(a.repeat)]
    emit({"mode": "logdet", "n": n, "probes": probes, "rank": rank, "steps": steps, "scan": scan, "estimate": out["estimate"],
          "std_error": out["std_error"], "logdet_precond": out["logdet_precond"], "ritz_min": out["ritz_min"], "ritz_max": out["ritz_max"],
          "logdet_pc_s": statistics.median(warm), "logdet_pc_with_setup_s": statistics.median(cold), "plain_steps": 100,
          "plain_estimate": plain["estimate"], "plain_std_error": plain["std_error"], "plain_logdet_s": statistics.median(t_plain),
          "numpy_slogdet": float(exact), "repeat": a.repeat}, a.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["step", "logdet"], required=True)
    ap.add_argument("--ns", type=int, nargs="+", default=[4096, 10000, 32768])
    ap.add_argument("--ks", type=int, nargs="+", default=[8])
    ap.add_argument("--ranks", type=int, nargs="+", default=[0, 16, 64, 256])
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
