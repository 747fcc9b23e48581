#!/usr/bin/env python3
"""Cost and gain of the pivoted-Cholesky preconditioner, in ONE process.

  ms per iteration: the device time of one cgx_solve_steps call (events around its kernels, steps_device_ms) / iterations, after a
    warm-up call; the median over --reps rounds in which the plain per-launch iteration (no preconditioner: the baseline) and
    rank 16 / 64 / 256 alternate on the same context.  The matrix is the generated one in dense storage (the cost of an iteration
    does not depend on the entries, and it keeps CG busy for any number of steps): N = 4096 and 10000 on the per-launch path,
    N = 32768 through 10821 and through variant 6 (gemv_variant -1).  Beside it the expectation from bytes for the general K1:
    (8 n^2 + 16 k n) / (8 n^2).
  plain_default_wall_ms: where the library's default for the plain solve is a persistent kernel (n <= 16384), its wall time per
    iteration, for the comparison a user of the default actually faces.
  set-up: the wall time of the first cgx_solve_begin with a rank minus that of a second one (which finds the factor made).
  iterations to tol = 1e-6 ||b|| on a kernel matrix A = S K S + sigma^2 I built with numpy (--kernel-n, default 4096; the recipe
    of tests/pivchol_reference.py) for plain CG, point Jacobi and every rank.

Prints one JSON object per line and appends them to profiles/pivchol/pivchol_bench.jsonl (--out).  Under rocprofv3 --kernel-trace
--stats the program goes after `--`."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402,F401  (first: libcgx binds to the HIP runtime torch loaded)
import __graft_entry__ as g  # noqa: E402

RANKS = (16, 64, 256)


def _begin_end(s, n):
    t0 = time.perf_counter()
    s.solve_begin(np.zeros(n))
    s.solve_steps(0)          # synchronises
    t1 = time.perf_counter()
    s.solve_end(np.zeros(n))
    return 1e3 * (t1 - t0)


def _kind(s, rank):
    if rank:
        s.set_preconditioner("pivchol", rank=rank)
    else:
        s.set_preconditioner(None)


def measure(pkg, n, variant, steps, warmup, reps):
    out = {"n": n, "gemv_variant": variant, "matrix": "lap2d"}
    with pkg.CGSolver(gemv_variant=variant, profile_gemv=True) as s:
        s.generate_lap2d_matrix(n)
        s.init_source_term(1.0 / n)
        s.tolerance(0.0)
        s.set_max_iter(warmup + steps)
        setup = {}
        for k in RANKS:
            _kind(s, k)
            first = _begin_end(s, n)
            setup[k] = first - _begin_end(s, n)
        kinds = (0,) + RANKS
        samples = {k: [] for k in kinds}
        for _ in range(reps):
            for k in kinds:   # every switch of the rank makes the factor again, outside the timed steps
                _kind(s, k)
                x = np.zeros(n)
                s.solve_begin(x)
                s.solve_steps(warmup)
                s.solve_steps(steps)
                res = s.solve_end(x)
                assert res["iterations"] == warmup + steps, res
                samples[k].append(res["steps_device_ms"] / steps)
        out["plan_variant"] = s.gemv_plan()["variant"]
        med = {k: statistics.median(samples[k]) for k in kinds}
        out["ms_per_iteration"] = med
        out["time_ratio_to_plain"] = {k: med[k] / med[0] for k in RANKS}
        out["expected_ratio_from_bytes"] = {k: (8.0 * n * n + 16.0 * k * n) / (8.0 * n * n) for k in RANKS}
        out["setup_ms"] = setup
        out["samples_ms"] = samples
    if n <= 16384 and not os.environ.get("CGX_RESIDENT") == "0":
        with pkg.CGSolver() as s:   # the plain solve as the library runs it by default at this size
            s.generate_lap2d_matrix(n)
            s.init_source_term(1.0 / n)
            s.tolerance(0.0)
            s.set_max_iter(warmup + steps)
            out["plain_default_plan_variant"] = s.gemv_plan()["variant"]
            wall = []
            for _ in range(reps):
                s.solve_begin(np.zeros(n))
                s.solve_steps(warmup)
                t0 = time.perf_counter()
                s.solve_steps(steps)
                wall.append(1e3 * (time.perf_counter() - t0) / steps)
                s.solve_end(np.zeros(n))
            out["plain_default_wall_ms"] = statistics.median(wall)
    return out


def count_iterations(pkg, n):
    import pivchol_reference as ref
    A, b = ref.kernel_matrix(n, 0.2, 1e-2)
    out = {"n": n, "matrix": "kernel, ell 0.2, sigma^2 1e-2", "tol": "1e-6 ||b||"}
    with pkg.CGSolver(gemv_variant=-1) as s:
        s.set_matrix_dense(A)
        s.set_source_term(b)
        s.tolerance(1e-6 * float(np.linalg.norm(b)))
        s.set_max_iter(20000)
        its = {}
        for name, kw in (("plain", None), ("jacobi", {"kind": "jacobi"})) + tuple(("rank %d" % k, {"kind": "pivchol", "rank": k}) for k in RANKS):
            if kw is None:
                s.set_preconditioner(None)
            else:
                s.set_preconditioner(**kw)
            res = s.solve(np.zeros(n))
            its[name] = res["iterations"] if res["converged"] else None
        out["iterations_to_tol"] = its
        out["iteration_ratio_plain_over_rank"] = {k: (its["plain"] / its["rank %d" % k] if its["plain"] and its["rank %d" % k] else None)
                                                  for k in RANKS}
        out["delta_used"] = s.preconditioner_shift()[1]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--skip-large", action="store_true", help="leave out N = 32768")
    ap.add_argument("--only", type=int, default=0, help="one size only")
    ap.add_argument("--kernel-n", type=int, default=4096, help="size of the kernel matrix of the iteration counts (0: none)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pivchol", "pivchol_bench.jsonl"))
    args = ap.parse_args()
    pkg = g.load_package()
    cases = [(4096, -1), (10000, -1)]
    if not args.skip_large:
        cases += [(32768, 10821), (32768, -1)]
    lines = []
    for n, v in cases:
        if args.only and n != args.only:
            continue
        lines.append(json.dumps(measure(pkg, n, v, args.steps, args.warmup, args.reps)))
        print(lines[-1], flush=True)
    if args.kernel_n and not args.only:
        lines.append(json.dumps(count_iterations(pkg, args.kernel_n)))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
