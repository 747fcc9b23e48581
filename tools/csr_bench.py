"""Opt-in CSR storage: K1 and K3 medians, time per iteration and K1 GB/s on gemv_bytes, for every forced
lane count L (gemv_variant 70000 + L) and the default, beside banded storage (direct form, 30001) where the matrix has a banded
form.  Not the BASELINE metric (bench.py measures the dense GEMV).

    python tools/csr_bench.py [--out FILE] [--sizes 20,24] [--only lap2d] [--configs default,30001]

Cases: the generated lap2d matrix, the same matrix randomly permuted (no banded form) and a skewed random SPD matrix (most rows
3-9 entries, 1 % of the rows 500-2000).  One JSON line per (case, n, config) on stdout."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402

pkg = g.load_package()
LANES = (1, 2, 4, 8, 16, 32, 64)


def lap2d_csr(n, perm=None):
    inc = int(np.floor(np.sqrt(n)))
    i = np.arange(n, dtype=np.int64)
    rows, cols, vals = [i], [i], [np.full(n, 4.0)]
    for off, ok in ((-1, i > 0), (1, i < n - 1), (-(inc + 1), i > inc), (inc + 1, i < n - 1 - inc)):
        rows.append(i[ok])
        cols.append(i[ok] + off)
        vals.append(np.full(int(ok.sum()), -1.0))
    r, c, v = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
    if perm is not None:
        r, c = perm[r], perm[c]
    order = np.lexsort((c, r))
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.add.at(indptr, r + 1, 1)
    return np.cumsum(indptr), c[order].astype(np.int32), v[order]


def skewed_spd(n, seed=7):
    rng = np.random.default_rng(seed)
    cnt = rng.integers(3, 10, n)
    heavy = rng.choice(n, n // 100, replace=False)
    cnt[heavy] = rng.integers(500, 2001, len(heavy))
    r = np.repeat(np.arange(n, dtype=np.int64), cnt)
    c = rng.integers(0, n, len(r))
    v = -rng.uniform(0.1, 1.0, len(r))
    keep = r != c
    lo, hi = np.minimum(r, c)[keep], np.maximum(r, c)[keep]   # summed once per unordered pair, then mirrored: exactly symmetric
    uk, inv = np.unique(lo * n + hi, return_inverse=True)
    half = np.zeros(len(uk))
    np.add.at(half, inv, v[keep])
    r, c, vals = np.concatenate([uk // n, uk % n]), np.concatenate([uk % n, uk // n]), np.concatenate([half, half])
    diag = np.zeros(n)
    np.add.at(diag, r, -vals)
    r, c, vals = np.concatenate([r, np.arange(n)]), np.concatenate([c, np.arange(n)]), np.concatenate([vals, diag + 1.0])
    order = np.lexsort((c, r))
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.add.at(indptr, r + 1, 1)
    return np.cumsum(indptr), c[order].astype(np.int32), vals[order]


def run(n, fmt, variant, csr=None, iters=200):
    with pkg.CGSolver(matrix_format=fmt, gemv_variant=variant, profile_gemv=1, profile_update=True) as s:
        if csr is None:
            s.generate_lap2d_matrix(n)
        else:
            s.set_matrix_csr(*csr)
        s.init_source_term(1.0 / n)
        s.set_max_iter(10 ** 9)
        s.tolerance(0.0)
        plan = s.gemv_plan()
        nnz = s.matrix_nnz()
        s.solve_begin(np.zeros(n))
        s.solve_steps(iters // 4)
        best, k1, k3 = 1e9, [], []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            s.solve_steps(iters)
            best = min(best, (time.perf_counter() - t0) / iters)
            k1.append(np.median(s.gemv_samples()))
            k3.append(np.median(s.update_samples()))
        r = s.solve_end()
    k1_us, k3_us = float(np.median(k1)) * 1e3, float(np.median(k3)) * 1e3
    return {"n": n, "format": "csr" if fmt == pkg.MATRIX_CSR else "banded", "variant": variant, "plan_variant": plan["variant"],
            "L": plan["R"] if fmt == pkg.MATRIX_CSR else None, "nnz": nnz, "k1_us": k1_us, "k3_us": k3_us,
            "us_per_iteration": best * 1e6, "gemv_bytes": r["gemv_bytes"], "k1_GBs": r["gemv_bytes"] / (k1_us * 1e-6) / 1e9}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default="20,24")
    ap.add_argument("--only", default="lap2d,permuted,skewed")
    ap.add_argument("--configs", default="")
    ap.add_argument("--iters", type=int, default=0, help="timed iterations per repetition (default 400 up to 2^20, else 100)")
    a = ap.parse_args()
    configs = [c for c in a.configs.split(",") if c] or (["30001", "default"] + ["7%04d" % L for L in LANES])
    rows = []
    for lg in [int(x) for x in a.sizes.split(",")]:
        n = 1 << lg
        iters = a.iters or (400 if lg <= 20 else 100)
        for case in a.only.split(","):
            if case == "skewed" and lg > 20:
                continue   # 1 % of the rows with 500-2000 entries: 2^20 rows already hold 19 M entries
            csr = None if case == "lap2d" else (lap2d_csr(n, np.random.default_rng(lg).permutation(n)) if case == "permuted"
                                                 else skewed_spd(n))
            for cfg in configs:
                if cfg == "30001":
                    if case != "lap2d":
                        continue   # no banded form
                    row = run(n, pkg.MATRIX_BANDED, 30001, iters=iters)
                else:
                    row = run(n, pkg.MATRIX_CSR, 0 if cfg == "default" else int(cfg), csr, iters=iters)
                row["case"] = case
                row["config"] = cfg
                rows.append(row)
                print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump({"rows": rows}, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
