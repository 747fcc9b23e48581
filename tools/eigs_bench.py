"""Extreme eigenpairs by Lanczos with full reorthogonalisation (cgx_eigenpairs): one JSON object per line.

--mode step      wall time per step of eigenpairs (8 largest, tol = 0) beside lanczos at one vector on the same context, alternated,
                 on the symmetric dense hash matrix (filled on the device) for every N and step count; medians over --repeat
                 alternated rounds behind a warm-up call of each.  Beside them the byte model: the reorthogonalisation reads the
                 basis four times per step, sum over t of 4 (t + 1) 8 n bytes against 8 n^2 of the mat-vec, 2 (m + 1) / n of it over
                 m steps; and the host's share of a call (the Ritz pairs: cgx_tridiag_eigenvectors on the same coefficients).
--mode trace     ONE eigenpairs call (8 largest, tol = 0, --steps-list[0] steps) at --ns[0] for a `rocprofv3 --kernel-trace --stats`
                 run of this program; the line carries the bytes the kernels stream.  --trace-csv FILE afterwards turns the kernel
                 trace of that run into durations and rates of the last 8 steps' projection and subtraction launches and of the
                 combine launch.
--mode tol       what the host's look at the Ritz estimates behind every 16th step costs: eigenpairs with tol = 1e-10 against
                 tol = 0 at the step count the first one ended with, on the kernel matrix of the tests at --workload-n, alternated.
--mode workload  one call on that kernel matrix: the 8 largest pairs with tol = 1e-10, wall time (median over --repeat calls behind a
                 warm-up call), steps, residuals, and the error against numpy.linalg.eigh with the host's time beside it.
"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SEED = 0x3D1F
NEV = 8


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


def mode_step(pkg, a):
    cgx = pkg.cgx
    for n in a.ns:
        with hash_solver(pkg, n) as s:
            v0 = np.random.default_rng(n).standard_normal(n)
            for steps in sorted(a.steps_list, reverse=True):      # the longest first: the basis block is made once
                alpha, beta, _ = s.lanczos(v0[None, :], steps)
                index = list(range(steps - 1, steps - 1 - NEV, -1))
                s.eigenpairs(NEV, "largest", steps, v0=v0)        # warm
                lz, eg, ho = [], [], []
                for _ in range(a.repeat):
                    lz.append(wall(lambda: s.lanczos(v0[None, :], steps)))
                    eg.append(wall(lambda: s.eigenpairs(NEV, "largest", steps, v0=v0)))
                    ho.append(wall(lambda: cgx.tridiag_eigenvectors(alpha[0], beta[0], index)))
                t_l, t_e, t_h = (statistics.median(v) for v in (lz, eg, ho))
                emit({"mode": "step", "n": n, "steps": steps, "nev": NEV, "lanczos_ms_per_step": 1e3 * t_l / steps,
                      "eigenpairs_ms_per_step": 1e3 * t_e / steps, "excess_fraction": t_e / t_l - 1.0,
                      "byte_model_fraction": 2.0 * (steps + 1) / n, "host_ritz_ms_per_call": 1e3 * t_h,
                      "excess_fraction_without_host_ritz": (t_e - t_h) / t_l - 1.0, "launches_per_step": 6, "repeat": a.repeat}, a.out)


def mode_trace(pkg, a):
    n, steps = a.ns[0], a.steps_list[0]
    with hash_solver(pkg, n) as s:
        v0 = np.random.default_rng(n).standard_normal(n)
        _, _, info = s.eigenpairs(NEV, "largest", steps, v0=v0)
    emit({"mode": "trace", "n": n, "steps": steps, "nev": NEV, "steps_done": info["steps_done"],
          "project_bytes_at_t": "8 n (t + 2)", "subtract_bytes_at_t": "8 n (t + 3)", "combine_bytes": 8 * n * (info["steps_done"] + NEV)}, a.out)


def mode_trace_csv(a):
    """Per-dispatch durations from rocprofv3's kernel trace of a --mode trace run."""
    n, steps = a.ns[0], a.steps_list[0]
    rows = {}
    with open(a.trace_csv) as f:
        for r in csv.DictReader(f):
            name = r["Kernel_Name"]
            for key in ("k_eigs_project<true>", "k_eigs_project<false>", "k_eigs_subtract<true>", "k_eigs_subtract<false>", "k_eigs_combine",
                        "k_eigs_normalise", "k_multi_gemv<1, false>"):
                if key in name:
                    rows.setdefault(key, []).append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    rec = {"mode": "trace_csv", "n": n, "steps": steps, "last": 8}
    for key, v in rows.items():
        v.sort()
        d = [ns for _, ns in v]
        last = d[-8:] if "combine" not in key else d
        us = statistics.median(last) / 1e3
        rec[key] = {"calls": len(d), "median_us_of_last": us, "mean_us_all": statistics.mean(d) / 1e3}
        t = steps - 4.5                                           # the middle of the last 8 steps
        if "project" in key:
            rec[key]["TBps"] = 8.0 * n * (t + 2) / (us * 1e-6) / 1e12
        elif "subtract" in key:
            rec[key]["TBps"] = 8.0 * n * (t + 3) / (us * 1e-6) / 1e12
        elif "combine" in key:
            rec[key]["TBps"] = 8.0 * n * (steps + NEV) / (us * 1e-6) / 1e12
        elif "gemv" in key:
            rec[key]["TBps"] = 8.0 * n * n / (us * 1e-6) / 1e12
    emit(rec, a.out)


def mode_tol(pkg, a):
    n = a.workload_n
    A = kernel_matrix(n)
    with pkg.CGSolver(gemv_variant=-1) as s:
        s.set_matrix_dense(A)
        _, _, info = s.eigenpairs(NEV, "largest", 256, tol=1e-10)
        m = info["steps_done"]
        s.eigenpairs(NEV, "largest", m)
        with_tol, without = [], []
        for _ in range(a.repeat):
            with_tol.append(wall(lambda: s.eigenpairs(NEV, "largest", 256, tol=1e-10)))
            without.append(wall(lambda: s.eigenpairs(NEV, "largest", m)))
    t1, t0 = statistics.median(with_tol), statistics.median(without)
    emit({"mode": "tol", "n": n, "nev": NEV, "steps_done": m, "looks": (m + 15) // 16, "tol_1e-10_ms": 1e3 * t1, "tol_0_ms": 1e3 * t0,
          "cost_of_the_looks_ms": 1e3 * (t1 - t0), "per_look_us": 1e6 * (t1 - t0) / max((m + 15) // 16, 1), "repeat": a.repeat}, a.out)


def mode_workload(pkg, a):
    n = a.workload_n
    A = kernel_matrix(n)
    t0 = time.perf_counter()
    lam, Q = np.linalg.eigh(A)
    t_host = time.perf_counter() - t0
    with pkg.CGSolver(gemv_variant=-1) as s:
        s.set_matrix_dense(A)
        vals, X, info = s.eigenpairs(NEV, "largest", 256, tol=1e-10)
        times = [wall(lambda: s.eigenpairs(NEV, "largest", 256, tol=1e-10)) for _ in range(a.repeat)]
    want, Xw = lam[::-1][:NEV], Q[:, ::-1][:, :NEV].T
    sign = np.where(np.sum(X * Xw, axis=1) < 0.0, -1.0, 1.0)
    emit({"mode": "workload", "n": n, "nev": NEV, "tol": 1e-10, "eigenpairs_s": statistics.median(times), "steps_done": info["steps_done"],
          "values": [float(v) for v in vals], "residual_over_norm": [float(r / lam[-1]) for r in info["residual"]],
          "estimate_over_norm": [float(e / lam[-1]) for e in info["estimate"]],
          "value_error_over_norm": [float(abs(v - w) / lam[-1]) for v, w in zip(vals, want)],
          "vector_error": [float(np.linalg.norm(sign[j] * X[j] - Xw[j])) for j in range(NEV)],
          "condition_number": float(lam[-1] / lam[0]), "numpy_eigh_host_s": t_host, "repeat": a.repeat}, a.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["step", "trace", "trace_csv", "tol", "workload"], required=True)
    ap.add_argument("--ns", type=int, nargs="+", default=[4096, 10000, 32768])
    ap.add_argument("--steps-list", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--workload-n", type=int, default=4096)
    ap.add_argument("--trace-csv", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.mode == "trace_csv":
        return mode_trace_csv(a)
    import torch  # noqa: F401  (first: libcgx then binds to the HIP runtime torch loaded)
    import __graft_entry__ as g
    pkg = g.load_package()
    {"step": mode_step, "trace": mode_trace, "tol": mode_tol, "workload": mode_workload}[a.mode](pkg, a)


if __name__ == "__main__":
    main()
