"""Several right-hand sides with a preconditioner (cgx_solve_multi_pc): one JSON object per line.

--mode iter   per-iteration time at tol = 0 and a fixed number of iterations behind a warmup solve, on the symmetric dense hash
              matrix (SPD by a dominant diagonal, filled on the device) for every N, rank and k: ms per iteration (the loop's wall
              time / iterations) and the event-timed median of K1m, of cgx_solve_multi_pc with the pivoted-Cholesky factor and,
              alternated in the same process on the same context, of the plain cgx_solve_multi at the same k; the median over
              --repeat runs of each.  Beside the ratio: the extra bytes the preconditioned iteration is known to move over A's
              (16 rank n for L in two launches, 32 k n for z and the second pass over r).
--mode solve  whole solves on the kernel matrix of the tests (n = 4096, tol = 1e-6 |b|, rank 64, k = 8): one cgx_solve_multi_pc
              against eight cgx_solve with the same factor on the same context and against one plain cgx_solve_multi; wall time
              around the calls (each ends in a device synchronise), the factor made before, medians over --repeat alternated runs.
--mode lreuse the same iterations through cgx_solve_multi_pc and through k single solves (n, rank, k, fixed iterations), for a
              run under `rocprofv3 --kernel-trace --stats -- python tools/multi_pc_bench.py --mode lreuse ...`: the stats table
              then holds k_multi_lr_update / k_multi_lr_apply beside k times k_lr_update / k_lr_apply.
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
    """A = S K S + sigma^2 I with a Gaussian kernel on uniform points of the unit square, s log-uniform in [1, 4]; b."""
    rng = np.random.default_rng(seed)
    pts = rng.random((n, 2))
    s = np.exp(rng.uniform(0.0, np.log(4.0), n))
    d2 = ((pts[:, None, :] - pts[None, :, :]) ** 2).sum(axis=2)
    A = s[:, None] * np.exp(-d2 / (2.0 * ell * ell)) * s[None, :]
    A = 0.5 * (A + A.T)
    A[np.diag_indices(n)] += sigma2
    return A, np.sin(0.37 * np.arange(n)) + 0.5


def rhs_block(A, b, k, seed=7):
    rng = np.random.default_rng(seed)
    n = len(b)
    cols = [b, np.cos(0.11 * np.arange(n)), rng.standard_normal(n), A @ rng.standard_normal(n)]
    while len(cols) < k:
        cols.append(rng.standard_normal(n) * (1.0 + len(cols)))
    return np.array(cols[:k])


def mode_iter(pkg, a):
    for n in a.ns:
        with pkg.CGSolver(gemv_variant=-1, profile_gemv=1) as s:
            s.generate_lap2d_matrix(n)
            s.probe_fill_matrix_hash(SEED, symmetric=True, diag=1.03 * 2.0 * np.sqrt(n / 3.0))
            s.tolerance(0.0)
            rng = np.random.default_rng(1)
            for k in a.ks:
                B = rng.standard_normal((k, n))

                def run(call):
                    s.set_max_iter(a.warmup)
                    call(B)
                    s.set_max_iter(a.steps)
                    _, res = call(B)
                    return 1e3 * res[0]["seconds_loop"] / a.steps, res[0]["gemv_ms_median"]

                for rank in a.ranks:
                    pc, plain = [], []
                    for _ in range(a.repeat):   # alternated: the same context, the same process
                        s.set_preconditioner("pivchol", rank=rank)
                        pc.append(run(s.solve_multi_pc))
                        s.set_preconditioner(None)
                        plain.append(run(s.solve_multi))
                    ms_pc, k1_pc = (statistics.median(v) for v in zip(*pc))
                    ms_pl, k1_pl = (statistics.median(v) for v in zip(*plain))
                    extra = (16.0 * rank * n + 32.0 * k * n) / (8.0 * n * n)
                    print(json.dumps({"mode": "iter", "n": n, "k": k, "rank": rank, "steps": a.steps, "repeat": a.repeat,
                                      "pc_ms_per_iteration": ms_pc, "plain_ms_per_iteration": ms_pl, "ratio": ms_pc / ms_pl,
                                      "pc_k1m_median_ms": k1_pc, "plain_k1m_median_ms": k1_pl, "k1m_ratio": k1_pc / k1_pl,
                                      "pc_update_ms": ms_pc - k1_pc, "plain_update_ms": ms_pl - k1_pl,
                                      "extra_bytes_over_a": extra,
                                      "pc_spread": [min(v[0] for v in pc), max(v[0] for v in pc)],
                                      "plain_spread": [min(v[0] for v in plain), max(v[0] for v in plain)]}), flush=True)


def mode_solve(pkg, a):
    n, k, rank = a.ns[0], a.ks[0], a.ranks[0]
    A, b = kernel_matrix(n)
    B = rhs_block(A, b, k)
    tol = 1e-6 * float(np.linalg.norm(b))
    with pkg.CGSolver(gemv_variant=-1) as s:
        s.set_matrix_dense(A)
        s.set_source_term(b)
        s.set_max_iter(20000)
        s.tolerance(tol)

        def multi_pc():
            s.set_preconditioner("pivchol", rank=rank)
            t = time.perf_counter()
            _, res = s.solve_multi_pc(B)
            return time.perf_counter() - t, [r["iterations"] for r in res], all(r["converged"] for r in res)

        def singles():
            s.set_preconditioner("pivchol", rank=rank)
            its, ok, t = [], True, 0.0
            for j in range(k):
                s.set_source_term(B[j])
                x = np.zeros(n)
                t0 = time.perf_counter()
                r = s.solve(x)
                t += time.perf_counter() - t0     # (the upload of b_j is outside: the multi call's upload of B is inside)
                its.append(r["iterations"])
                ok = ok and bool(r["converged"])
            return t, its, ok

        def multi_plain():
            s.set_preconditioner(None)
            t = time.perf_counter()
            _, res = s.solve_multi(B)
            return time.perf_counter() - t, [r["iterations"] for r in res], all(r["converged"] for r in res)

        for f in (multi_pc, singles, multi_plain):   # warm up every shape; the factor is made here
            f()
        runs = {"multi_pc": [], "singles": [], "multi_plain": []}
        for _ in range(a.repeat):
            for name, f in (("multi_pc", multi_pc), ("singles", singles), ("multi_plain", multi_plain)):
                runs[name].append(f())
        out = {"mode": "solve", "n": n, "k": k, "rank": rank, "tol": tol, "repeat": a.repeat}
        for name, v in runs.items():
            out[name + "_s"] = statistics.median(t for t, _, _ in v)
            out[name + "_spread_s"] = [min(t for t, _, _ in v), max(t for t, _, _ in v)]
            out[name + "_iterations"] = v[0][1]
            out[name + "_converged"] = all(ok for _, _, ok in v)
        out["singles_over_multi_pc"] = out["singles_s"] / out["multi_pc_s"]
        out["multi_plain_over_multi_pc"] = out["multi_plain_s"] / out["multi_pc_s"]
        print(json.dumps(out), flush=True)


def mode_lreuse(pkg, a):
    n, k = a.ns[0], a.ks[0]
    A, b = kernel_matrix(n)
    B = rhs_block(A, b, k)
    with pkg.CGSolver(gemv_variant=-1) as s:
        s.set_matrix_dense(A)
        s.set_source_term(b)
        s.tolerance(0.0)
        s.set_max_iter(a.steps)
        for rank in a.ranks:
            s.set_preconditioner("pivchol", rank=rank)
            for _ in range(1 + a.repeat):
                s.solve_multi_pc(B)
                for j in range(k):
                    s.set_source_term(B[j])
                    s.solve(np.zeros(n))
            print(json.dumps({"mode": "lreuse", "n": n, "k": k, "rank": rank, "steps": a.steps, "solves_of_each": 1 + a.repeat}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("iter", "solve", "lreuse"), default="iter")
    ap.add_argument("--ns", default=None)
    ap.add_argument("--ks", default=None)
    ap.add_argument("--ranks", default=None)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeat", type=int, default=5)
    a = ap.parse_args()
    defaults = {"iter": ("4096,10000,32768", "1,4,8,16", "16,64,256"), "solve": ("4096", "8", "64"), "lreuse": ("4096", "8", "64")}[a.mode]
    a.ns = [int(v) for v in (a.ns or defaults[0]).split(",")]
    a.ks = [int(v) for v in (a.ks or defaults[1]).split(",")]
    a.ranks = [int(v) for v in (a.ranks or defaults[2]).split(",")]
    import torch  # noqa: F401  (libcgx binds to the HIP runtime torch loaded)
    import __graft_entry__ as g
    pkg = g.load_package()
    {"iter": mode_iter, "solve": mode_solve, "lreuse": mode_lreuse}[a.mode](pkg, a)


if __name__ == "__main__":
    main()
