"""Several right-hand sides against one matrix (cgx_solve_multi): one JSON line.

At N = 32768, tol = 0 and a fixed number of iterations after a warmup solve, on the generated (lap2d) and the dense hash matrix,
for k = 1, 2, 4, 8, 16: the multi-vector K1's event-timed median (K1m), ms per iteration (the loop's wall time / iterations),
column-iterations per second and A-bytes per second (8 n^2 per iteration).  Alternated in the same process: the single path's
K1 median with gemv_variant 10821 (bench.py's explicit shape).  Usage: python tools/multi_rhs_bench.py [--n N] [--steps K]
[--warmup W] [--ks 1,2,4,8,16]."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=32768)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ks", default="1,2,4,8,16")
    a = ap.parse_args()
    import torch  # noqa: F401  (libcgx binds to the HIP runtime torch loaded)
    import __graft_entry__ as g
    pkg = g.load_package()
    n, ks = a.n, [int(v) for v in a.ks.split(",")]
    out = {"n": n, "steps": a.steps, "warmup": a.warmup, "matrices": {}}
    for kind in ("lap2d", "hash"):
        rows = []
        with pkg.CGSolver(gemv_variant=10821, profile_gemv=1) as s1, pkg.CGSolver(gemv_variant=-1, profile_gemv=1) as sm:
            for s in (s1, sm):
                s.generate_lap2d_matrix(n)
                if kind == "hash":
                    s.probe_fill_matrix_hash(0x3D1F, symmetric=False, diag=0.0)
                s.tolerance(0.0)
            s1.init_source_term(1.0 / n)
            rng = np.random.default_rng(1)
            for k in ks:
                B = rng.standard_normal((k, n))
                sm.set_max_iter(a.warmup)
                sm.solve_multi(B)
                sm.set_max_iter(a.steps)
                _, res = sm.solve_multi(B)
                s1.set_max_iter(a.steps)
                r1 = s1.solve(np.zeros(n))
                ms_iter = 1e3 * res[0]["seconds_loop"] / a.steps
                rows.append({"k": k, "k1m_median_ms": res[0]["gemv_ms_median"], "ms_per_iteration": ms_iter,
                             "column_iterations_per_s": k * 1e3 / ms_iter, "a_bytes_per_s": 8.0 * n * n * 1e3 / ms_iter,
                             "k1m_a_bytes_per_s": 8.0 * n * n * 1e3 / res[0]["gemv_ms_median"],
                             "single_k1_median_ms": r1["gemv_ms_median"],
                             "iteration_over_single_k1": ms_iter / r1["gemv_ms_median"]})
        out["matrices"][kind] = rows
    print(json.dumps(out))


if __name__ == "__main__":
    main()
