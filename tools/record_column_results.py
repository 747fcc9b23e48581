#!/usr/bin/env python3
"""What the four k-column solves (solve_multi, solve_multi_pc, solve_shifted, solve_minres) return on a fixed set of small
problems, bit for bit: one JSON object, case name -> {"x_sha256": digest of X's bytes, "results": one dict per column}.

Every field of every result dict is kept except the wall and event times (seconds_*, gemv_ms_*); floats are written by
float.hex(), so equality of the file is equality of the bits.  These solves add in fixed orders and use no floating-point atomics
(DESIGN.md), so a recording made at one commit is what every later commit must reproduce: tests/test_gpu_column_norms.py runs
record() and compares it with tests/golden/column_results_parent.json, which this tool wrote at the commit in front of the one
that folded the solves' verification norms and result fillers into one (python tools/record_column_results.py --out FILE).

The problems: the symmetric hash matrix with a dominant diagonal at n = 1000 (less than one trip of the 1024-thread norms kernel,
idle lanes, no multiple of 64), 1025 (one thread makes a second trip) and 2500 (an uneven third trip); on CSR storage the same
matrix cut to the band |i - j| <= BAND.  max_iter is 40 at most and the tolerance absolute, so that of the columns of a case --
right-hand sides of different scale, shifts of different size -- some converge and some run out.
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x5EED
SIZES = (1000, 1025, 2500)
MAX_ITER, TOL = 40, 1e-6
BAND, CSR_MAX_ITER = 40, 8
SCALES = (1.0, 1e-4, 1e-7)                          # of the right-hand sides of a multi solve, cycling
SHIFTS_3 = [0.0, 0.5, 4.0]
SHIFTS_16 = [0.0, 0.25, 0.5, 1.0, 2.0, 3.0, 4.0, 6.0, 8.0, 12.0, 16.0, 24.0, 32.0, 48.0, 64.0, 96.0]
SHIFTS_CSR = [0.0, 0.5, 40.0]
MINRES_3 = [0.0, -0.3, 2.0]
MINRES_16 = [0.0, -0.3, 2.0, -8.0, 0.25, -3.0, 4.0, -0.9, 8.0, -20.0, 16.0, 1.0, 32.0, -50.0, 64.0, 0.5]
MINRES_CSR = [0.0, -0.3, 40.0]
TIMINGS = ("seconds_", "gemv_ms_")


def diag_of(n):
    return 1.03 * 2.0 * np.sqrt(n / 3.0)             # beyond the spectral radius of the off-diagonal part


def source(n):
    return np.cos(np.arange(n, dtype=np.float64))


def rhs_block(n, k):
    i = np.arange(n, dtype=np.float64)
    return np.array([SCALES[j % len(SCALES)] * np.cos(0.37 * (j + 1) * i + j) for j in range(k)])


def dense_solver(pkg, n, b, max_iter=MAX_ITER):
    s = pkg.CGSolver(gemv_variant=-1)
    s.generate_lap2d_matrix(n)
    s.probe_fill_matrix_hash(SEED, symmetric=True, diag=diag_of(n))
    s.set_source_term(b)
    s.set_max_iter(max_iter)
    s.tolerance(TOL)
    return s


def band_csr(A):
    """(indptr, indices, data) of A cut to |i - j| <= BAND."""
    n = A.shape[0]
    i, j = np.nonzero(np.abs(np.subtract.outer(np.arange(n), np.arange(n))) <= BAND)   # row-major: columns ascending in a row
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.add.at(indptr, i + 1, 1)
    return np.cumsum(indptr), j.astype(np.int32), A[i, j]


def csr_solver(pkg, n, csr):
    s = pkg.CGSolver(gemv_variant=-1, matrix_format=pkg.MATRIX_CSR)
    s.set_matrix_csr(*csr, n)
    s.set_source_term(source(n))
    s.set_max_iter(CSR_MAX_ITER)
    s.tolerance(TOL)
    return s


def entry(X, res):
    def enc(v):
        return float(v).hex() if isinstance(v, float) else int(v)
    return {"x_sha256": hashlib.sha256(np.ascontiguousarray(X).tobytes()).hexdigest(),
            "results": [{k: enc(v) for k, v in r.items() if not k.startswith(TIMINGS)} for r in res]}


def record(pkg):
    out = {}
    for n in SIZES:
        with dense_solver(pkg, n, source(n)) as s:
            for k in (1, 3, 16):
                out["n%d/multi/nrhs%d" % (n, k)] = entry(*s.solve_multi(rhs_block(n, k)))
            for name, kw in (("jacobi", {}), ("pivchol", {"rank": 8})):
                s.set_preconditioner(name, **kw)
                out["n%d/multi_pc/%s/nrhs3" % (n, name)] = entry(*s.solve_multi_pc(rhs_block(n, 3)))
            s.set_preconditioner(None)
            for name, sig in (("1", [0.0]), ("3", SHIFTS_3), ("16", SHIFTS_16)):
                out["n%d/shifted/dense/%s" % (n, name)] = entry(*s.solve_shifted(sig))
            for name, sig in (("3", MINRES_3), ("16", MINRES_16)):
                out["n%d/minres/dense/%s" % (n, name)] = entry(*s.solve_minres(sig))
            s.set_max_iter(0)
            out["n%d/minres/dense/max_iter0" % n] = entry(*s.solve_minres(MINRES_3))
            s.set_source_term(np.zeros(n))
            out["n%d/minres/dense/max_iter0_b0" % n] = entry(*s.solve_minres(MINRES_3))
            csr = band_csr(s.probe_matrix_rows()[0])
        with csr_solver(pkg, n, csr) as s:
            out["n%d/shifted/csr/3" % n] = entry(*s.solve_shifted(SHIFTS_CSR))
            out["n%d/minres/csr/3" % n] = entry(*s.solve_minres(MINRES_CSR))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "column_results_parent.json"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch  # noqa: F401  (first: libcgx then binds to the HIP runtime torch loaded)
    import __graft_entry__ as g
    rec = record(g.load_package())
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    for name, e in sorted(rec.items()):
        print(name, [(r["iterations"], r["converged"]) for r in e["results"]])


if __name__ == "__main__":
    main()
