#!/usr/bin/env python3
"""Cost of multi-shift CG beside the plain per-launch iteration, in ONE process.

  ms per iteration: the device time of the loop (events around its kernels, steps_device_ms) / iterations at tol = 0 and a fixed
    iteration count; per round a plain cgx_solve (the baseline) and cgx_solve_shifted with S = 1, 4, 16 shifts alternate on the
    same context, after one untimed round of each; medians and the spread (min, max) over --reps rounds.  Two shift sets: "wide"
    = spread over [0, 100] -- there zeta of the larger shifts falls below 2^-500 inside the window and the guard freezes them,
    so the later iterations update fewer vectors (shifts_frozen_in_window says how many) -- and "live" = spread over [0, 1e-3],
    where every shift runs for the whole window: the full cost of S shifts.
    N = 4096 and 32768 dense (generated lap2d, gemv_variant -1: 32768 runs the symmetric K1, variant 6) and lap2d 2^20 on CSR.
    The window at N = 4096 is 2000 iterations (about 45 ms) and no longer: at tol = 0 r.r of this matrix reaches the denormals
    after about 2900 iterations and is exactly 0 after 3012, beta turns into 0 / 0, the guard freezes every shift and the loop
    ends early (solves_shorter_than_window counts such samples; it must be 0).
  shift kernel: (ms per iteration of S shifts - plain) and the bytes it moves, 8 n (1 + 4 S); its own duration comes from a
    separate run under rocprofv3 --kernel-trace --stats (the program goes after `--`; use --steps 100 --reps 1 there).
  end to end (N = 32768 only): the iterations every shift of 16 needs to tol = 1e-10 from ONE converged cgx_solve_shifted per
    shift set, and from them and the measured ms per iteration: one shifted solve against 16 separate plain solves (computed,
    and labelled so; building and uploading 16 shifted matrices is not in it).

Prints one JSON object per line."""
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

COUNTS = (1, 4, 16)


SETS = {"wide": 100.0, "live": 1e-3}


def shifts_for(count, top=100.0):
    return [0.0] if count == 1 else list(np.linspace(0.0, top, count))


def measure(pkg, n, steps, reps, csr, converged, sets):
    out = {"n": n, "storage": "csr" if csr else "dense", "steps": steps, "reps": reps}
    fmt = pkg.MATRIX_CSR if csr else pkg.MATRIX_DENSE
    # profile_gemv: the loop's device window is recorded when K1 profiling is on; one K1 sample per call is all it adds
    with pkg.CGSolver(gemv_variant=0 if csr else -1, matrix_format=fmt, profile_gemv=1 << 30) as s:
        s.generate_lap2d_matrix(n)
        s.init_source_term(1.0 / n)
        s.tolerance(0.0)
        s.set_max_iter(steps)
        out["plan_variant"] = s.gemv_plan()["variant"]

        def plain():
            res = s.solve(np.zeros(n))
            short.append(res["iterations"] != steps)
            return res["steps_device_ms"] / steps

        frozen, short = {}, []   # short: a solve that did not run the whole window (then its sample is not a full one)

        def shifted(count, name):
            X, res = s.solve_shifted(shifts_for(count, SETS[name]))
            short.append(res[0]["iterations"] != steps)   # sigma = 0 is the seed: it runs the whole window
            frozen["%s_%d" % (name, count)] = sum(1 for r in res if r["converged"])
            return res[0]["steps_device_ms"] / steps

        cases = [("live", 1)] + [(name, c) for name in sets for c in COUNTS if c > 1]
        plain()
        for name, c in cases:
            shifted(c, name)
        samples = {"plain": [], **{"%s_%d" % (name, c): [] for name, c in cases}}
        for _ in range(reps):
            samples["plain"].append(plain())
            for name, c in cases:
                samples["%s_%d" % (name, c)].append(shifted(c, name))
        med = {k: statistics.median(v) for k, v in samples.items()}
        out["ms_per_iteration"] = med
        out["spread_ms"] = {k: [min(v), max(v)] for k, v in samples.items()}
        out["extra_us_over_plain"] = {k: 1e3 * (med[k] - med["plain"]) for k in med if k != "plain"}
        out["ratio_to_plain"] = {k: med[k] / med["plain"] for k in med if k != "plain"}
        out["shifts_frozen_in_window"] = frozen
        out["shift_kernel_bytes"] = {c: 8.0 * n * (1 + 4 * c) for c in COUNTS}
        # all of the extra time charged to the shift kernel's bytes (launch gap included: a lower bound of the kernel's own rate)
        out["live_bytes_over_extra_time_GBs"] = {c: 8.0 * n * (1 + 4 * c) / (1e6 * (med["live_%d" % c] - med["plain"]))
                                                 for c in COUNTS if "live_%d" % c in med and med["live_%d" % c] > med["plain"]}
        out["samples_ms"] = samples
        out["solves_shorter_than_window"] = sum(short)
        if converged:
            s.tolerance(1e-10)
            s.set_max_iter(n)
            out["converged"] = {}
            for name in sets:
                sig = shifts_for(16, SETS[name])
                X, res = s.solve_shifted(sig)
                its = [r["iterations"] + 1 for r in res]   # loop bodies run
                c = out["converged"][name] = {
                    "shifts": sig, "all_converged": all(r["converged"] for r in res), "loop_bodies": its,
                    "rel_residual": [r["rel_residual"] for r in res], "seconds_loop_measured": res[0]["seconds_loop"],
                    "computed_one_shifted_solve_ms": max(its) * med["%s_16" % name],
                    "computed_16_separate_solves_ms": sum(its) * med["plain"],
                }
                c["computed_speedup"] = c["computed_16_separate_solves_ms"] / c["computed_one_shifted_solve_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=0, help="iterations per timed solve (0: 400 at N = 32768 and on CSR, 2000 at 4096)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", type=int, default=0, help="one size only")
    ap.add_argument("--no-converged", action="store_true")
    ap.add_argument("--sets", default="wide,live", help="shift sets to run: wide (over [0, 100]), live (over [0, 1e-3])")
    args = ap.parse_args()
    pkg = g.load_package()
    sets = [name for name in args.sets.split(",") if name in SETS]
    for n, csr, steps in ((4096, False, 2000), (32768, False, 400), (1 << 20, True, 400)):
        if args.only and n != args.only:
            continue
        print(json.dumps(measure(pkg, n, args.steps or steps, args.reps, csr, n == 32768 and not args.no_converged, sets)),
              flush=True)


if __name__ == "__main__":
    main()
