"""The walk of the symmetric K1 (plan variant 6) in the REAL kernels, the grids interleaved in one process on one matrix:
CGX_SYMV_RUN = 0 (4 workgroups per CU, what gemv_variant 60000 runs), 4, 2, 1 tiles per workgroup.  Every rewrite of the matrix
plans again (plan_symmetric reads the variable), the 8 GiB block stays where it is; per round and run one
cgx_probe_time_gemv(REPS): ms per plain product = tile kernel + fold back to back.  One JSON line per run.
   python tools/symv_walk_ab.py [n] [rounds] [reps]"""
import json, os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g
pkg = g.load_package()
n = int(sys.argv[1]) if len(sys.argv) > 1 else 32768
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 40
runs = (0, 4, 2, 1)
ms = {r: [] for r in runs}
plans = {}
with pkg.CGSolver(gemv_variant=-1) as s:
    s.generate_lap2d_matrix(n)
    for rnd in range(rounds + 1):          # round 0 warms up
        for r in runs:
            os.environ["CGX_SYMV_RUN"] = str(r)
            s.probe_fill_matrix_hash(20261019, symmetric=True)
            plans[r] = s.gemv_plan()
            assert plans[r]["variant"] == 6, plans[r]
            t = s.probe_time_gemv(reps)
            if rnd:
                ms[r].append(round(t, 5))
for r in runs:
    print(json.dumps({"n": n, "run": r, "grid": plans[r]["grid"], "U": plans[r]["U"], "reps": reps,
                      "median_ms": float(np.median(ms[r])), "min_ms": min(ms[r]), "max_ms": max(ms[r]), "rounds_ms": ms[r]}), flush=True)
