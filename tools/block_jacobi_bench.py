#!/usr/bin/env python3
"""Cost and gain of block Jacobi, in ONE process.

  ms per iteration: the device time of one cgx_solve_steps call (events around its kernels, steps_device_ms) / iterations, after a
    warm-up call; the median over --reps rounds in which block = 1 (today's point-Jacobi kernels: the baseline) and every block of
    {4, 32, 64, 256} alternate on the same context.  N = 32768 through 10821 and through variant 6 (gemv_variant -1 on the
    generated matrix), N = 4096 / 8192 / 10000 on the per-launch path, and lap2d 2^20 on CSR storage.
  set-up: the wall time of the first cgx_solve_begin with a block size minus that of a second one (which finds the inverses made):
    extraction, exchange and inversion of the blocks.
  iterations to tol = 1e-6 ||b|| (b = init_source_term) for every block, where the size allows a full solve in reasonable time.

Prints one JSON object per line.  Under rocprofv3 --kernel-trace --stats the program goes after `--`."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402,F401  (first: libcgx binds to the HIP runtime torch loaded)
import __graft_entry__ as g  # noqa: E402

BLOCKS = (1, 4, 32, 64, 256)


def _begin_end(s, n):
    t0 = time.perf_counter()
    s.solve_begin(np.zeros(n))
    s.solve_steps(0)          # synchronises
    t1 = time.perf_counter()
    s.solve_end(np.zeros(n))
    return 1e3 * (t1 - t0)


def measure(pkg, n, variant, steps, warmup, reps, csr, count_iterations):
    out = {"n": n, "gemv_variant": variant, "storage": "csr" if csr else "dense"}
    fmt = pkg.MATRIX_CSR if csr else pkg.MATRIX_DENSE
    with pkg.CGSolver(gemv_variant=variant, matrix_format=fmt, profile_gemv=True) as s:
        s.generate_lap2d_matrix(n)
        s.init_source_term(1.0 / n)
        s.tolerance(0.0)
        s.set_max_iter(warmup + steps)
        setup = {}
        for b in BLOCKS:
            s.set_preconditioner("jacobi", block=b)
            first = _begin_end(s, n)
            setup[b] = first - _begin_end(s, n)
        samples = {b: [] for b in BLOCKS}
        for _ in range(reps):
            for b in BLOCKS:   # every switch of the block size makes the inverses again, outside the timed steps
                s.set_preconditioner("jacobi", block=b)
                x = np.zeros(n)
                s.solve_begin(x)
                s.solve_steps(warmup)
                s.solve_steps(steps)
                res = s.solve_end(x)
                assert res["iterations"] == warmup + steps, res
                samples[b].append(res["steps_device_ms"] / steps)
        out["plan_variant"] = s.gemv_plan()["variant"]
        med = {b: statistics.median(samples[b]) for b in BLOCKS}
        out["ms_per_iteration"] = med
        out["ratio_to_block_1"] = {b: med[b] / med[1] for b in BLOCKS}
        out["setup_ms"] = setup
        out["samples_ms"] = samples
        if count_iterations:
            tol = 1e-6 * float(np.linalg.norm(s.probe_source_term()))
            s.tolerance(tol)
            s.set_max_iter(n)
            its = {}
            for b in BLOCKS:
                s.set_preconditioner("jacobi", block=b)
                res = s.solve(np.zeros(n))
                its[b] = res["iterations"] if res["converged"] else None
            out["iterations_to_tol"] = its
            out["iteration_ratio_block_1_over_b"] = {b: (its[1] / its[b] if its[1] and its[b] else None) for b in BLOCKS}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--skip-large", action="store_true", help="leave out N = 32768 and the CSR problem")
    ap.add_argument("--only", type=int, default=0, help="one size only")
    args = ap.parse_args()
    pkg = g.load_package()
    cases = [(4096, -1, False, True), (8192, -1, False, True), (10000, -1, False, True)]
    if not args.skip_large:
        cases += [(32768, 10821, False, False), (32768, -1, False, False), (1 << 20, 0, True, False)]
    for n, v, csr, count in cases:
        if args.only and n != args.only:
            continue
        print(json.dumps(measure(pkg, n, v, args.steps, args.warmup, args.reps, csr, count)), flush=True)


if __name__ == "__main__":
    main()
