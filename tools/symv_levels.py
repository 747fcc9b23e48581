"""Where do the two time levels of the symmetric K1's step (N = 32768: about 0.66 and 0.72 ms) come from?  SOLVERS contexts alive
at once in ONE process, each with its own 8 GiB matrix (generate_lap2d_matrix, the benchmark's data), timed in turn for ROUNDS
rounds: STEPS fused iterations behind a warm-up, wall clock around cgx_solve_steps as bench.py takes it.
  - a level that belongs to a context (its allocations) shows as one context always slow, another always fast;
  - a level that belongs to the time (clocks) shows as all contexts changing together from round to round;
  - a level that belongs to the process shows as every figure of a process on one level.
One JSON line per round; at the end one sample of the clocks under load where rocm-smi is there to be asked.
   python tools/symv_levels.py [n] [solvers] [rounds] [steps]"""
import json, os, subprocess, sys, threading, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g
pkg = g.load_package()
n = int(sys.argv[1]) if len(sys.argv) > 1 else 32768
nsolvers = int(sys.argv[2]) if len(sys.argv) > 2 else 3
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 6
steps = int(sys.argv[4]) if len(sys.argv) > 4 else 300
variant = int(os.environ.get("VARIANT", "-1"))


def timed(s, k):
    s.set_max_iter(50 + k); s.tolerance(0.0); s.solve_begin(np.zeros(n)); s.solve_steps(50)
    torch.cuda.synchronize(); t0 = time.perf_counter(); s.solve_steps(k); torch.cuda.synchronize(); t1 = time.perf_counter()
    s.solve_end()
    return (t1 - t0) / k * 1e3


solvers = []
for i in range(nsolvers):
    s = pkg.CGSolver(gemv_variant=variant); s.generate_lap2d_matrix(n); s.init_source_term(1.0 / n); solvers.append(s)
plan = solvers[0].gemv_plan()
t_start = time.perf_counter()
for s in solvers:
    timed(s, 100)
for r in range(rounds):
    ms = [round(timed(s, steps), 5) for s in solvers]
    print(json.dumps({"pid": os.getpid(), "round": r, "t_s": round(time.perf_counter() - t_start, 2), "variant": plan["variant"],
                      "grid": plan["grid"], "ms_per_step": ms}), flush=True)
box = {}
def ask():
    try:
        box["out"] = subprocess.run(["rocm-smi", "--showclocks", "--showpower", "--json"], capture_output=True, text=True, timeout=20).stdout
    except Exception as e:   # noqa: BLE001
        box["out"] = "rocm-smi: %s" % e
th = threading.Thread(target=ask); th.start()
ms = []
while th.is_alive() and len(ms) < 40:
    ms.append(round(timed(solvers[0], steps), 5))
th.join()
print(json.dumps({"pid": os.getpid(), "under_load_ms_per_step": ms}), flush=True)
print(box.get("out", "").strip()[:6000], flush=True)
for s in solvers:
    s.close()
