#!/usr/bin/env python3
"""Cost of an iteration with and without the Jacobi preconditioner, in ONE process, plain and Jacobi solves
alternating on the same context, and iterations to tolerance on an S L S matrix.

  ms per iteration: the device time of one cgx_solve_steps call (events around its kernels, steps_device_ms) / iterations, after a
    warm-up call; the median over --reps alternating pairs.  N = 32768 through 10821 and through variant 6 (gemv_variant -1 on the
    generated matrix), N = 4096 / 8192 on the per-launch path.
  iterations to tolerance: A = S L S (L = lap2d, s_i in [1, 100]), b = init_source_term, tol = 1e-6 ||b||: plain CG on L, Jacobi and
    plain CG on S L S.

Prints one JSON object per line.  Under rocprofv3 --kernel-trace --stats the program goes after `--`."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402,F401  (first: libcgx binds to the HIP runtime torch loaded)
import __graft_entry__ as g  # noqa: E402


def per_iteration(pkg, n, variant, steps, warmup, reps):
    out = {"n": n, "gemv_variant": variant}
    with pkg.CGSolver(gemv_variant=variant, profile_gemv=True) as s:
        s.generate_lap2d_matrix(n)
        s.init_source_term(1.0 / n)
        s.tolerance(0.0)
        s.set_max_iter(warmup + steps)
        samples = {None: [], "jacobi": []}
        for _ in range(reps):
            for kind in (None, "jacobi"):
                s.set_preconditioner(kind)
                x = np.zeros(n)
                s.solve_begin(x)
                s.solve_steps(warmup)
                s.solve_steps(steps)
                res = s.solve_end(x)
                assert res["iterations"] == warmup + steps, res
                samples[kind].append(res["steps_device_ms"] / steps)
        out["plan_variant"] = s.gemv_plan()["variant"]
    out["plain_ms_per_iteration"] = statistics.median(samples[None])
    out["jacobi_ms_per_iteration"] = statistics.median(samples["jacobi"])
    out["ratio"] = out["jacobi_ms_per_iteration"] / out["plain_ms_per_iteration"]
    out["extra_us"] = 1e3 * (out["jacobi_ms_per_iteration"] - out["plain_ms_per_iteration"])
    out["samples_ms"] = {"plain": samples[None], "jacobi": samples["jacobi"]}
    return out


def sls_iterations(pkg, oracle, n):
    L = oracle.generate_lap2d(n)
    sc = np.geomspace(1.0, 100.0, n)[np.random.default_rng(20261015).permutation(n)]
    A = (sc[:, None] * L) * sc[None, :]
    tol = 1e-6 * float(np.linalg.norm(oracle.init_source_term(n)))
    out = {"n": n, "tol": tol, "max_iter": 4 * n}
    for name, M, kind in (("plain_L", L, None), ("jacobi_SLS", A, "jacobi"), ("plain_SLS", A, None)):
        with pkg.CGSolver(gemv_variant=-1) as s:
            s.set_preconditioner(kind)
            s.set_matrix_dense(M)
            s.init_source_term(1.0 / n)
            s.tolerance(tol)
            s.set_max_iter(4 * n)
            res = s.solve(np.zeros(n))
        out[name] = {"iterations": res["iterations"], "converged": res["converged"]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-large", action="store_true", help="leave out N = 32768")
    args = ap.parse_args()
    pkg = g.load_package()
    oracle = g.load_oracle()
    cases = [] if args.skip_large else [(32768, 10821), (32768, -1)]
    cases += [(4096, -1), (8192, -1)]
    for n, v in cases:
        print(json.dumps(per_iteration(pkg, n, v, args.steps, args.warmup, args.reps)), flush=True)
    for n in (1024, 4096):
        print(json.dumps(sls_iterations(pkg, oracle, n)), flush=True)


if __name__ == "__main__":
    main()
