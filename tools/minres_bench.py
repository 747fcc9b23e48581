"""MINRES (cgx_solve_minres) against multi-shift CG (cgx_solve_shifted, section 14): one JSON object per line.

The time of one iteration of either solver at 1 and at 16 shifts on the same context, alternated, on

  dense   the symmetric dense hash matrix (SPD by a dominant diagonal, filled on the device), n = 32768, the library's plan
          (variant 6, the symmetric upper-triangle K1);
  csr     the generator's lap2d in CSR storage, n = 2^22.

Both are wall-time differences between a long and a short call (--long / --short iterations at tol = 0) divided by the difference
in iterations, so the uploads, downloads, set-up launches and the final verification cancel; medians over --repeat alternated
rounds.  The shifts are small and positive, so that both solvers take them and none freezes; the iterations every shift reports
are recorded (a frozen shift would make the figure meaningless).
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


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def wall(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def problem(pkg, kind, n):
    if kind == "dense":
        s = pkg.CGSolver(gemv_variant=0)
        s.generate_lap2d_matrix(n)
        s.probe_fill_matrix_hash(SEED, symmetric=True, diag=1.03 * 2.0 * np.sqrt(n / 3.0))
        s.set_source_term(np.cos(np.arange(n, dtype=np.float64)))
    else:
        s = pkg.CGSolver(gemv_variant=-1, matrix_format=pkg.MATRIX_CSR)
        s.generate_lap2d_matrix(n)
        s.init_source_term(1.0 / n)
    s.tolerance(0.0)
    return s


def run(pkg, a, kind, n):
    with problem(pkg, kind, n) as s:
        plan = s.gemv_plan()
        for k in a.ks:
            shifts = [0.5 + 0.05 * j for j in range(k)]
            ran = {}

            def call(name, iters):
                s.set_max_iter(iters)
                t, (_, res) = wall(lambda: (s.solve_minres if name == "minres" else s.solve_shifted)(shifts))
                ran[name, iters] = sorted({r["iterations"] for r in res})
                return t

            per = {"minres": [], "shifted": []}
            for name in per:
                call(name, a.short)   # warm-up: side blocks, first-use set-up
            for _ in range(a.repeat):
                for name in per:
                    per[name].append((call(name, a.long) - call(name, a.short)) / (a.long - a.short))
            ms = {name: 1e3 * statistics.median(v) for name, v in per.items()}
            emit({"problem": kind, "n": n, "plan_variant": plan["variant"], "shifts": k, "minres_ms_per_iteration": ms["minres"],
                  "shifted_ms_per_iteration": ms["shifted"], "ratio": ms["minres"] / ms["shifted"],
                  "iterations_reported": {"%s_%d" % key: v for key, v in ran.items()}, "short": a.short, "long": a.long,
                  "repeat": a.repeat}, a.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", nargs="+", choices=["dense", "csr"], default=["dense", "csr"])
    ap.add_argument("--dense-n", type=int, default=32768)
    ap.add_argument("--csr-n", type=int, default=1 << 22)
    ap.add_argument("--ks", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--short", type=int, default=20)
    ap.add_argument("--long", type=int, default=120)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch  # noqa: F401  (first: libcgx then binds to the HIP runtime torch loaded)
    import __graft_entry__ as g
    pkg = g.load_package()
    for kind in a.problems:
        run(pkg, a, kind, a.dense_n if kind == "dense" else a.csr_n)


if __name__ == "__main__":
    main()
