#!/usr/bin/env python3
"""bench.py -- CG iterations/s and K1 HBM-roofline fraction on MI355X (BASELINE.json metric).

    python bench.py                       # 1 GPU, generate_lap2d N=32768, 500 timed iterations (configs[2])
    python bench.py --gpus N --steps K --warmup W       # row-block over N GPUs (configs[3], strong scaling): starts its
                                                        # own N ranks (one fresh child process per GPU, see self_launch)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W          # the same under an external launcher (RANK / WORLD_SIZE set)

A "step" is one body of the CG loop (code/MPI/cg.cc:96-137 of the reference): one A.p GEMV over this
rank's row block, two dot products, the x/r/p updates and the exchanges (here: ONE per iteration).  Inputs are synthetic and
HBM-resident before the timed region: A = generate_lap2d_matrix(N) built on the device, b = init_source_term(1/N).
W warmup steps, then exactly K steps between barrier + torch.cuda.synchronize() on both sides; every rank's clock runs from
the leading barrier to the end of its own synchronize, the MAX over ranks (= when the last rank finished) is the job's
time; rank 0 prints ONE JSON line.  value = K / t for the whole job (every rank advances the same K iterations).

Extra objects in the line:
  roofline     -- K1 (the GEMV) against the 8 TB/s HBM peak: algorithmic bytes 8*(rows*N + N + rows) per launch
                  divided by the MEDIAN launch duration of the timed region, measured with HIP events bound to the K1
                  dispatches on the library's own stream (the first launch after the sync is never a sample).
                  roofline.traffic = HBM bytes per K1 launch by PMC counters: on one GPU counted on THIS box by two
                  rocprofv3 --pmc child passes of the same workload after the timed region, else the committed row of
                  profiles/k1_hbm_traffic.json for the same K1 plan, else null.
  cpu_baseline -- the CPU oracle (oracle/cg_oracle.c, a port of the reference's serial path) run for a few
                  iterations of the same workload on one host core (rank 0, after the timed region, at any N).
  solve_window -- the same K iterations through the reference's own timing window (all of solve(), cg_main.cc:53-55).

--dump-outputs DIR: rank 0 writes what the timed run handed back after its last step (W + K iterations from x0 = 0): the
solution x (float64, length N) and residual_prev, x_norm and iterations (float64, one element each), as DIR/<name>.npy.
The inputs depend only on the arguments, so two builds can be compared output for output.

Rank 0 ALWAYS prints a line: if no transport produces a result, if an exception escapes, or if a watchdog expires, the line
has "value": null and an "error" object.
"""
import argparse
import csv
import glob
import json
import math
import os
import re
import shutil
import signal
import socket
import subprocess
import sys
import tempfile
import threading
import time
import traceback

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0   # MI355X HBM3E spec peak, /opt/skills/guides/MI355X_MICROARCH.md "Chip-level parameters"
TRAFFIC_FILE = "profiles/k1_hbm_traffic.json"


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=500)      # BASELINE.json configs[2]: fixed 500 iterations
    ap.add_argument("--warmup", type=int, default=100)   # ~0.12 s: lets the clocks settle before the timed region
    ap.add_argument("--matrix-size", dest="n", type=int, default=0, help="matrix size (default 32768; weak mode: floor(16384*sqrt(P)))")
    ap.add_argument("--mode", choices=["strong", "weak"], default="strong")
    ap.add_argument("--variant", type=int, default=0, help="K1 shape override (DESIGN.md)")
    ap.add_argument("--transport", choices=["auto", "p2p-tag", "p2p", "p2p-sep", "rccl"], default="auto",
                    help="multi-GPU exchange: direct xGMI mailboxes with the exchange folded into K3 -- bytes handed over as "
                         "tagged 8-byte words (p2p-tag) or as payload + flag words (p2p) -- or as its own kernel (p2p-sep), RCCL, "
                         "or whichever of those works and calibrates fastest on this node (auto)")
    ap.add_argument("--lda-pad", type=int, default=-1)
    ap.add_argument("--cpu-baseline-iters", type=int, default=20)   # 20-50 loop bodies at N=32768, not 500
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-profile-gemv", action="store_true", help="do not time K1 with HIP events")
    ap.add_argument("--profile-every", type=int, default=0,
                    help="event-time every n-th K1 launch (default: when steps <= 64 every launch on one GPU, so that a "
                         "short window still gives >= 16 samples, every 4th on several; else 4 on one GPU, 8 on several)")
    ap.add_argument("--profile-update", action="store_true",
                    help="also event-time the update kernel (K3, or K3 with the exchange inside) on the launches whose K1 is timed; "
                         "default: on for several GPUs (its duration then holds the wait for the peers = the cost of the exchange), "
                         "off on one (a timed dispatch costs ~5 us of stream time)")
    ap.add_argument("--no-solve-window", action="store_true", help="skip the extra untimed solve() through the reference's window")
    ap.add_argument("--no-live-pmc", action="store_true",
                    help="do not collect K1's HBM traffic with two rocprofv3 --pmc child passes of this program (one GPU only, "
                         "after the timed region; ~20 s); roofline.traffic then comes from the committed file or is null")
    ap.add_argument("--wireup-timeout", type=float, default=float(os.environ.get("CGX_BENCH_WIREUP_TIMEOUT", "90")),
                    help="seconds one transport's wire-up stage may take before that transport is dropped")
    ap.add_argument("--watchdog", type=float, default=float(os.environ.get("CGX_BENCH_WATCHDOG", "480")),
                    help="seconds after which rank 0 prints a failure line and the process exits")
    ap.add_argument("--no-dense-check", action="store_true",
                    help="skip the dense-data leg (after the timed region: the same K1 on a matrix in which every element is a "
                         "different number -- roofline.dense_random; ~K more iterations)")
    # tests only (tests/test_gpu_bench.py): "<transport>:<stage>" or "extra:cpu baseline" never comes back.  An explicit
    # argument, not an environment variable: nothing in a user's environment changes what the benchmark does.
    ap.add_argument("--no-reference-sizes", action="store_true",
                    help="skip the extra `reference_sizes` (one GPU, after the measurement: iterations/s at the reference's own "
                         "sizes N = 1024, 2048 and 4096, the resident persistent kernel beside the per-launch path; ~1 s)")
    ap.add_argument("--dump-outputs", metavar="DIR", default="",
                    help="after the timed steps, write what they computed (x, residual, ||x||, iterations) as DIR/<name>.npy")
    ap.add_argument("--test-hang", default="", help=argparse.SUPPRESS)
    return ap.parse_args()


def pmc_traffic(n, nranks, plan):
    """HBM bytes per K1 launch from a committed rocprofv3 --pmc pass (profiles/), or None.  A row counts only if it was
    collected on the SAME K1 form (R, U, light, split as the library reports them for this run) at the same n and shard
    count: a counter file of another kernel is no evidence for this one."""
    path = os.path.join(ROOT, TRAFFIC_FILE)
    try:
        rows = json.load(open(path))["rows"]
    except Exception:
        return None
    want = {k: int(plan[k]) for k in ("R", "U", "light", "split")} if plan else None
    for r in rows:
        if r.get("n") == n and r.get("nranks") == nranks and want is not None and \
                {k: int(r.get("plan", {}).get(k, -1)) for k in want} == want:
            return r.get("hbm_bytes_per_launch")
    return None


K1_FUSED = re.compile(r"k_gemv_colsplit<\d+, \d+, \d+, 1(?:, (?:true|false))*>|k_gemv_ldsp<\d+, \d+, \d+, 1>")


def live_pmc_traffic(args, n):
    """K1's HBM bytes per launch ON THIS BOX, NOW: two short child runs of this same program under rocprofv3 --pmc -- FETCH_SIZE,
    then WRITE_SIZE, separate passes with --kernel-trace only, corrected as /opt/skills/guides/MI355X_MICROARCH.md prescribes
    (on gfx950 FETCH_SIZE counts the 128-B requests of a wide coalesced read at 64 B: read bytes = FETCH_SIZE x 1024 x 2;
    WRITE_SIZE x 1024 is exact).  One GPU only.  Returns (bytes per launch or None, note)."""
    exe = shutil.which("rocprofv3")
    if exe is None:
        return None, "rocprofv3 not on PATH"
    if any(k.startswith(("ROCP_", "ROCPROF")) for k in os.environ) or "rocprof" in os.environ.get("LD_PRELOAD", ""):
        return None, "this process already runs under a profiler"
    means, launches = {}, 0
    for counter in ("FETCH_SIZE", "WRITE_SIZE"):
        d = tempfile.mkdtemp(prefix="cgx_pmc_", dir="/tmp")
        try:
            cmd = [exe, "--pmc", counter, "--kernel-trace", "--output-format", "csv", "-d", d, "--", sys.executable,
                   os.path.abspath(__file__), "--steps", "20", "--warmup", "5", "--matrix-size", str(n), "--variant", str(args.variant),
                   "--lda-pad", str(args.lda_pad), "--no-cpu-baseline", "--no-solve-window", "--no-live-pmc", "--no-profile-gemv", "--no-reference-sizes"]
            env = {k: v for k, v in os.environ.items()           # the child is a plain one-GPU run, never a rank of somebody's job
                   if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE", "GROUP_RANK", "ROLE_RANK", "MASTER_ADDR",
                                "MASTER_PORT", "TORCHELASTIC_RUN_ID")}
            # its own process group, known to stop_launched(): on a timeout, the watchdog or SIGTERM the profiler AND the
            # bench.py under it (which holds an 8 GiB matrix on the GPU this process still uses) are ended together
            proc = subprocess.Popen(cmd, cwd="/tmp", env=dict(env, TMPDIR="/tmp"), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                                    text=True, start_new_session=True)
            LAUNCHED["extra"] = proc
            try:
                _, err = proc.communicate(timeout=100)
            except subprocess.TimeoutExpired:
                stop_group(proc)
                return None, "rocprofv3 --pmc %s pass did not finish within 100 s (its process group was ended)" % counter
            finally:
                LAUNCHED["extra"] = None
            files = glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True)
            if proc.returncode != 0 or not files:
                return None, "rocprofv3 --pmc %s pass failed (rc %d): %s" % (counter, proc.returncode, (err or "")[-300:])
            vals = [float(row["Counter_Value"]) for row in csv.DictReader(open(files[0]))
                    if row["Counter_Name"] == counter and K1_FUSED.search(row["Kernel_Name"])]
            if not vals:
                return None, "no K1 dispatch in the %s pass" % counter
            means[counter], launches = sum(vals) / len(vals), len(vals)
        except Exception as e:                     # noqa: BLE001 -- a measurement aid must never cost the line
            return None, "%s pass: %s" % (counter, str(e)[:200])
        finally:
            shutil.rmtree(d, ignore_errors=True)
    return means["FETCH_SIZE"] * 1024 * 2 + means["WRITE_SIZE"] * 1024, "%d K1 launches per pass" % launches


def broadcast_bytes(dist, payload, nbytes, device):
    """Rank 0's `payload` (bytes of length nbytes) to every rank of the default process group."""
    import torch
    if dist.get_rank() == 0:
        assert len(payload) == nbytes
        t = torch.tensor(list(payload), dtype=torch.uint8, device=device)
    else:
        t = torch.zeros(nbytes, dtype=torch.uint8, device=device)
    dist.broadcast(t, src=0)
    return bytes(t.cpu().tolist())


def call_with_timeout(fn, seconds, what):
    """fn() on a helper thread, at most `seconds`.  A call that does not come back (a hung ncclCommInitRank, a peer
    that never opens its mailbox) raises TimeoutError here; the helper thread is abandoned (daemon) and the process
    leaves through os._exit at the end, so it can never hold the driver's limit."""
    box = {}

    def body():
        try:
            box["value"] = fn()
        except BaseException as e:          # noqa: BLE001 -- re-raised on the calling thread
            box["error"] = e

    t = threading.Thread(target=body, daemon=True, name="bench-" + what)
    t.start()
    t.join(seconds)
    if t.is_alive():
        raise TimeoutError("%s did not finish within %.0f s" % (what, seconds))
    if "error" in box:
        raise box["error"]
    return box.get("value")


def cpu_baseline_iters(n, asked):
    """Loop bodies to time: the asked count at N <= 32768, fewer above (the cost of one body grows with N^2), at least 3."""
    return max(3, min(asked, int(asked * (32768.0 / n) ** 2))) if n > 32768 else asked


def cpu_baseline(n, iters):
    import __graft_entry__ as g
    O = g.load_oracle()
    iters = cpu_baseline_iters(n, iters)
    t0 = time.time()
    _, r = O.solve_lap2d(n, iters, 0.0, 1)     # tol 0: never converges, exactly `iters` loop bodies
    wall = time.time() - t0
    out = {
        "value": iters / r["seconds_loop"], "unit": "iterations/s", "cores": 1, "kind": "port",
        "sample": "oracle/cg_oracle.c serial CG, generate_lap2d N=%d, %d of the loop bodies timed (loop only, "
                  "%.1f s; %.1f s incl. building the 8*N^2-byte matrix)" % (n, iters, r["seconds_loop"], wall),
        "gemv_GBs": 8.0 * n * n * iters / r["seconds_loop"] / 1e9,
    }
    try:
        model = [l.split(":", 1)[1].strip() for l in open("/proc/cpuinfo") if l.startswith("model name")][0]
    except Exception:
        model = "unknown"
    out["host_cpu"] = model
    out["host_cores_available"] = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    # context row: all host cores of this box's share, row blocks = threads = the
    # reference's MPI ranks; same arithmetic, bit-identical result
    try:
        cores = min(len(os.sched_getaffinity(0)), 16)
    except AttributeError:
        cores = min(os.cpu_count() or 1, 16)
    if cores > 1:
        O.set_threads(cores)
        _, ra = O.solve_lap2d(n, iters, 0.0, cores)
        O.set_threads(1)
        out["all_cores"] = {"value": iters / ra["seconds_loop"], "unit": "iterations/s", "cores": cores, "kind": "port",
                            "sample": "same, %d row blocks on %d threads" % (cores, cores),
                            "gemv_GBs": 8.0 * n * n * iters / ra["seconds_loop"] / 1e9}
    # context row: the GEMV of the loop (99 % of it, figures/gprof.png) through the BLAS family the reference linked -- the OpenBLAS
    # that numpy / scipy bundle, held to ONE thread -- on the same matrix: what cblas_dgemv (cg.cc:101-102) itself does on this host
    try:
        import numpy as np
        from scipy.linalg import blas
        from threadpoolctl import threadpool_limits
        A = O.generate_lap2d(n)
        v = O.init_source_term(n)
        reps = max(3, iters // 2)
        with threadpool_limits(limits=1, user_api="blas"):
            blas.dgemv(1.0, A.T, v, trans=1)
            t0 = time.time()
            for _ in range(reps):
                y = blas.dgemv(1.0, A.T, v, trans=1)
            dt = time.time() - t0
        ver = ""
        try:
            from threadpoolctl import threadpool_info
            ver = ", ".join(sorted({"%s %s" % (i.get("internal_api"), i.get("version")) for i in threadpool_info() if i.get("user_api") == "blas"}))
        except Exception:                  # noqa: BLE001
            pass
        out["openblas_gemv_1thread"] = {"value": reps / dt, "unit": "GEMVs/s (one per iteration)", "cores": 1, "gemv_GBs": 8.0 * n * n * reps / dt / 1e9,
                                        "sample": "%d x dgemv of the %d x %d matrix through scipy.linalg.blas (%s), one thread" % (reps, n, n, ver or "OpenBLAS"),
                                        "checksum": float(np.sum(y))}
        del A
    except Exception as e:                 # noqa: BLE001 -- context only
        out["openblas_gemv_1thread"] = {"skipped": str(e)[:120]}
    return out


def reference_sizes(pkg, torch):
    """The reference's own experiment sizes (code/MPI/cg.run:15-44: N = 1024, 2048, 4096, 8192 ... to convergence or 200 iterations)
    and BASELINE.json configs[1]'s N = 10000 on this GPU: iterations/s of the loop with the library's default (n <= 4096: the resident
    persistent kernel; n <= 10000: the streaming persistent kernel, section 4c; above: K1 + K3) and with the
    per-launch path (K1 + K3 per iteration), tol = 0, timed iterations after 200, best of 3; `hbm_roofline_frac` = the whole
    iteration against the GEMV's algorithmic bytes 8 (n^2 + 2 n) at 8 TB/s.  Not the headline metric."""
    import numpy as np
    rows = []
    for n in (1024, 2048, 4096, 8192, 10000):
        row = {"n": n}
        steps = 2000 if n <= 4096 else 600
        for name, variant in (("default", 0), ("per_launch", -1)):
            with pkg.CGSolver(gemv_variant=variant) as s:
                s.generate_lap2d_matrix(n)
                s.set_max_iter(10 ** 8)
                s.tolerance(0.0)
                s.init_source_term(1.0 / n)
                plan = s.gemv_plan()
                s.solve_begin(np.zeros(n))
                s.solve_steps(200)
                best = float("inf")
                for _ in range(3):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    s.solve_steps(steps)
                    best = min(best, (time.perf_counter() - t0) / steps)
                s.solve_end()
            row[name] = {"iterations_per_s": 1.0 / best, "us_per_iteration": best * 1e6,
                         "hbm_roofline_frac": 8.0 * (n * n + 2 * n) / best / (HBM_PEAK_GBS * 1e9),
                         "kernel": ("one persistent kernel, A in LDS" + (" + registers + streamed rest" if plan["light"] else ""))
                         if plan["variant"] == 4 else "one persistent kernel, A streamed" if plan["variant"] == 5 else "K1 + K3 per iteration"}
        rows.append(row)
    return rows


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(out_dir, x, res):
    """--dump-outputs: the arrays a caller of the timed path receives, as out_dir/<name>.npy (float64).  Returns the names."""
    import numpy as np
    arrays = {"x": np.ascontiguousarray(x, dtype=np.float64)}
    for k in ("residual_prev", "x_norm", "iterations"):
        arrays[k] = np.array([res[k]], dtype=np.float64)
    total = sum(a.nbytes for a in arrays.values())
    if total > DUMP_LIMIT_BYTES:
        raise RuntimeError("--dump-outputs: %d bytes exceed the %d byte limit" % (total, DUMP_LIMIT_BYTES))
    os.makedirs(out_dir, exist_ok=True)
    for k, a in arrays.items():
        np.save(os.path.join(out_dir, k + ".npy"), a)
    return sorted(arrays)


def problem_size(args, world):
    if args.n:
        return args.n
    if args.mode == "weak":
        return int(math.floor(16384 * math.sqrt(world)))   # code/MPI/cg.run:22-44 rounding rule, N^2/P constant
    return 32768


def base_line(args, world, n):
    """The fields of the line that do not depend on a measurement (also the body of a failure line)."""
    return {
        "metric": "cg_iterations_per_sec",
        "value": None,
        "unit": "iterations/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": None,
        "higher_is_better": True,
        "scaling": args.mode,
        "vs_baseline": None,           # the reference publishes seconds only, nothing at this N
        "dtype": "f64",
        "data": "synthetic",
        "config": {
            "workload": "generate_lap2d_matrix N=%d, init_source_term(1/N), fixed-iteration dense fp64 CG "
                        "(BASELINE.json configs[%d])" % (n, 4 if args.mode == "weak" else (2 if world == 1 else 3)),
            "n": n, "parallelism": "rowblock%d" % world,
        },
    }


class Bench:
    """One rank of the measurement.  Every decision that changes the sequence of torch.distributed calls is taken on a
    rank-reduced value (all_ok), so a local failure can never leave the ranks inside different collectives."""

    def __init__(self, args, world, rank, local_rank, state):
        self.args, self.world, self.rank, self.local_rank, self.state = args, world, rank, local_rank, state
        self.dist = None
        self.ctl = "cuda"       # device of the small control-plane tensors
        self.n = problem_size(args, world)
        self.notes = []
        self.prewarm_iterations = {}
        self.gpu_work_s = 0.0          # seconds of solver work this rank put on its GPU (pre-warm, calibration, timed run, window)
        self.gpu_iterations = 0
        self.update_samples = []       # durations (ms) of the event-timed update kernels of the most recent run()
        self.last_x = None             # the solution x of the most recent run()
        self.rccl_nranks = None        # ncclCommCount of the RCCL candidate (min over ranks), if one was built

    # ---- plumbing ------------------------------------------------------------------------------------
    def log(self, msg):
        print("bench.py rank %d: %s" % (self.rank, msg), file=sys.stderr, flush=True)

    def all_ok(self, flag):
        """True only if `flag` is true on every rank (so that all ranks take the same branch)."""
        if self.dist is None:
            return bool(flag)
        t = self.torch.tensor([1 if flag else 0], dtype=self.torch.int32, device=self.ctl)
        self.dist.all_reduce(t, op=self.dist.ReduceOp.MIN)
        return bool(t.item())

    def sync(self):
        if self.dist is not None:
            self.dist.barrier()
        self.torch.cuda.synchronize()
        if self.dist is not None:
            self.dist.barrier()

    def gather_rows(self, values):
        """Every rank's list of floats -> list over ranks (rank order)."""
        torch = self.torch
        mine = torch.tensor(values, dtype=torch.float64, device=self.ctl)
        if self.dist is None:
            return [mine.cpu().tolist()]
        allv = [torch.zeros_like(mine) for _ in range(self.world)]
        self.dist.all_gather(allv, mine)
        return [v.cpu().tolist() for v in allv]

    def gather_strings(self, text, width=32):
        raw = text.encode()[:width].ljust(width, b"\0")
        rows = self.gather_rows([float(b) for b in raw])
        return [bytes(int(b) for b in r).rstrip(b"\0").decode(errors="replace") for r in rows]

    # ---- set-up ---------------------------------------------------------------------------------------
    def init(self):
        self.state["stage"] = "import torch / init_process_group"
        import numpy as np
        import torch   # before libcgx: the library then shares the HIP/RCCL instances torch loaded
        import __graft_entry__ as g
        self.np, self.torch, self.g = np, torch, g
        args, world, rank = self.args, self.world, self.rank

        assert torch.cuda.is_available(), "bench.py needs an MI355X; there is no CPU path to time"
        ndev = torch.cuda.device_count()
        self.backend = os.environ.get("CGX_BENCH_BACKEND", "nccl")   # "gloo": rehearsal of world > 1 on a one-GPU box
        if world > ndev and self.backend == "nccl":
            # every rank sees the same count and leaves here, before any rendezvous: a clean failure line, not a hang
            raise RuntimeError("bench.py --gpus %d needs %d MI355X, %d visible here (CGX_BENCH_BACKEND=gloo rehearses several "
                               "ranks on one GPU over the IPC mailboxes)" % (world, world, ndev))
        if self.local_rank >= ndev:
            # more ranks than GPUs is only ever a rehearsal on a one-GPU box (RCCL itself refuses duplicate devices)
            self.local_rank = self.local_rank % ndev
        torch.cuda.set_device(self.local_rank)
        self.pkg = g.load_package()

        # Under torch.distributed.run (RANK set) the RCCL path is used even for one rank, so that the launcher
        # plumbing and the collectives can be rehearsed on a one-GPU box; plain `python bench.py` has no comm.
        self.use_comm = world > 1 or ("RANK" in os.environ and os.environ.get("CGX_BENCH_FORCE_SELF") != "1")
        if self.use_comm:
            import torch.distributed as dist

            def init_pg():
                if self.backend == "nccl":
                    dist.init_process_group(backend="nccl", rank=rank, world_size=world,
                                            device_id=torch.device("cuda", self.local_rank))
                else:
                    dist.init_process_group(backend=self.backend, rank=rank, world_size=world)
            call_with_timeout(init_pg, max(self.args.wireup_timeout, 120.0), "init_process_group")
            if self.backend != "nccl":
                self.ctl = "cpu"
            self.dist = dist
        if args.no_profile_gemv:
            self.profile_every = 0
        elif args.profile_every:
            self.profile_every = args.profile_every
        else:
            # a timed dispatch costs ~4.5 us of stream time (measured, tools/window_short.sh: a 181 us iteration -- what a
            # rank of an 8-GPU run has -- slows by 2.6 % with every K1 timed, 5.6 % with the update kernel timed as well,
            # 0.3 % with every 4th): every launch on one GPU's 1.2 ms iteration, every 4th one (plus the update kernel of the
            # same iterations) where the iteration is a fraction of that
            self.profile_every = (1 if world == 1 else 4) if args.steps <= 64 else (4 if world == 1 else 8)

    def make_solver(self, transport):
        """transport: 'self' | 'rccl' | 'p2p-tag' | 'p2p' | 'p2p-sep'.  Returns a ready solver or None (same answer on every rank).
        The wire-up is cut into stages; after each one all ranks agree (all_ok) whether to go on, so that a failure on
        one rank can never leave the others inside a different torch.distributed call.  Every stage that can block on a
        peer is bounded by --wireup-timeout."""
        pkg, dist, world, rank, n, args = self.pkg, self.dist, self.world, self.rank, self.n, self.args
        # the metric and its roofline are defined on the per-launch path (K1 = the dense GEMV kernel): -1 keeps it also for a
        # --matrix-size of 4096 or less, where the library's default would be the resident persistent kernel (reported
        # separately as `reference_sizes`)
        common = dict(nranks=world, rank=rank, device=self.local_rank, gemv_variant=args.variant or -1, lda_pad=args.lda_pad,
                      profile_gemv=self.profile_every, profile_update=bool(self.profile_every) and (world > 1 or args.profile_update))
        box = {"s": None, "uid": None, "handle": None}
        self.state["stage"] = "wire-up of transport " + transport

        def stage(what, fn, bounded=True):
            ok = True
            if bounded and args.test_hang == "%s:%s" % (transport, what):
                inner = fn                            # test hook (tests/test_gpu_bench.py): this stage never comes back

                def fn():                             # noqa: F811
                    time.sleep(3600)
                    return inner()
            try:
                ok = (call_with_timeout(fn, args.wireup_timeout, "%s/%s" % (transport, what)) if bounded else fn()) is not False
            except BaseException as e:               # noqa: BLE001 -- any failure means "do not use this transport"
                if isinstance(e, TimeoutError):
                    box["stuck"] = True              # a helper thread may still be inside the library with this context
                self.log("transport %s unavailable (%s): %s" % (transport, what, e))
                self.notes.append("%s dropped at '%s' on rank %d: %s" % (transport, what, rank, str(e)[:200]))
                ok = False
            return self.all_ok(ok)

        def give_up():
            if box["s"] is not None and not box.get("stuck"):   # never destroy a context another thread may be using
                try:
                    box["s"].close()
                except Exception:                    # noqa: BLE001
                    pass
            return None

        if transport == "self":
            def create():
                box["s"] = pkg.CGSolver(comm_mode=pkg.COMM_SELF, **common)
            if not stage("create", create, bounded=False):
                return give_up()
        elif transport == "rccl":
            # replaces mpirun's wire-up (MPI_Init, cg_main.cc:15-20): every rank gets rank 0's RCCL id
            def make_id():
                box["uid"] = pkg.comm_unique_id() if rank == 0 else None
            if not stage("unique id", make_id):
                return give_up()
            uid = broadcast_bytes(dist, box["uid"], pkg.cgx.UNIQUE_ID_BYTES, self.ctl)

            def create():
                box["s"] = pkg.CGSolver(comm_mode=pkg.COMM_RCCL, unique_id=uid, **common)
            if not stage("ncclCommInitRank", create):
                return give_up()
        else:
            def create():
                box["s"] = pkg.CGSolver(comm_mode=pkg.COMM_P2P, p2p_separate_exchange=(transport == "p2p-sep"),
                                        p2p_tagged=(transport == "p2p-tag"), **common)
                box["handle"] = box["s"].p2p_export()
            if not stage("mailbox allocation", create):
                return give_up()
            torch = self.torch
            mine = torch.tensor(list(box["handle"]), dtype=torch.uint8, device=self.ctl)
            allh = [torch.zeros_like(mine) for _ in range(world)]
            dist.all_gather(allh, mine)              # every rank's mailbox handle to every rank

            def attach():
                box["s"].p2p_import(b"".join(bytes(t.cpu().tolist()) for t in allh))
            if not stage("opening the peers' mailboxes", attach):   # also the barrier: every rank has attached
                return give_up()

            def selftest():
                return bool(box["s"].p2p_selftest(32))   # pattern all-gathers, verified, every wait bounded
            if not stage("self-test", selftest):
                return give_up()

        # The problem is set up ONCE per solver: re-allocating the 8 GiB matrix after a free can land on
        # fragmented memory and cost ~3 % of K1 (measured), so calibration and timed run share one allocation.
        def problem():
            box["s"].generate_lap2d_matrix(n)
            box["s"].init_source_term(1.0 / n)
        if not stage("problem set-up", problem, bounded=False):
            return give_up()
        return box["s"]

    # ---- the measurement ------------------------------------------------------------------------------
    def run(self, s, warmup, steps):
        """W warm-up + K timed loop bodies on solver s.  Returns (elapsed, result, samples) or None.  Every rank makes
        the same sequence of torch.distributed calls whatever fails locally, so a failure cannot desynchronise."""
        np, torch, dist, n = self.np, self.torch, self.dist, self.n
        ok = True
        x = np.zeros(n)
        try:
            s.set_max_iter(warmup + steps)
            s.tolerance(0.0)               # fixed-iteration run: the break of cg.cc:120 is never taken
            s.solve_begin(x)
            s.solve_steps(warmup)
        except Exception as e:             # noqa: BLE001
            self.log("warm-up failed: %s" % e)
            ok = False
        if not self.all_ok(ok):
            return None
        self.sync()
        t0 = time.perf_counter()
        try:
            s.solve_steps(steps)           # enqueues K loop bodies and synchronises the library's stream
        except Exception as e:             # noqa: BLE001
            self.log("timed steps failed: %s" % e)
            ok = False
        torch.cuda.synchronize()
        elapsed = time.perf_counter() - t0     # this rank's K steps are done; the MAX over ranks below is the job's time
        self.gpu_work_s += elapsed
        self.gpu_iterations += warmup + steps
        if dist is not None:
            dist.barrier()                     # closes the bracket; its own latency (a collective launch) is not CG work
        res, samples = None, None
        try:
            samples = s.gemv_samples() if self.profile_every else np.zeros(0)
            self.update_samples = s.update_samples() if self.profile_every else np.zeros(0)
            res = s.solve_end(x)
            self.last_x = x
        except Exception as e:             # noqa: BLE001
            self.log("solve_end failed: %s" % e)
            ok = False
        if ok and dist is not None:
            # every rank must have reached bit-identical scalars (a stale or torn exchange would break this)
            allv = self.gather_rows([res["iterations"], res["residual_prev"], res["x_norm"]])
            if not all(v == allv[0] for v in allv) or not math.isfinite(res["residual_prev"]):
                self.log("ranks disagree on the result")
                ok = False
        elif dist is not None:
            self.gather_rows([0.0, 0.0, 0.0])
        if not self.all_ok(ok):
            return None
        return elapsed, res, samples

    def prewarm(self, s, tname):
        """Untimed: the same iteration in windows of about a quarter of a second until two successive windows take
        the same time to 0.4 % (clocks settled; a box that has just been powered up needs longer than a warm one), at
        least two and at most eight windows.  A window is cut into solves that stay below the iteration count at which
        this matrix converges (~5.6 sqrt(N): with tol = 0 the recurrence would run on into 0/0).  All lengths are
        computed, not measured, and the stop decision is taken on the max over ranks, so every rank does the same
        number of exchanges."""
        est = 8.0 * self.n * self.n / max(self.world, 1) / 6.5e12 + 25e-6
        iters = max(25, min(10000, int(0.25 / est)))
        chunk = max(10, min(iters, int(2.5 * math.sqrt(self.n))))
        prev, total = None, 0
        for _ in range(8):
            t, left = 0.0, iters
            while left > 0:
                k = min(chunk, left)
                out = self.run(s, 0, k)
                if out is None:
                    return False
                t += self.max_over_ranks(out[0])
                left -= k
            total += iters
            if prev is not None and abs(t - prev) <= 0.004 * t:
                break
            prev = t
        self.prewarm_iterations[tname] = total
        return True

    def max_over_ranks(self, v):
        return max(r[0] for r in self.gather_rows([v]))

    def solve_window(self, s, steps):
        """The same K iterations through the reference's own timing window: ONE solve() call, timed inside the library
        from its first to its last statement (cg_main.cc:53-55 times all of CGSolver::solve: set-up, the initial
        residual GEMV, the loop, the gather of x and the DEBUG verification GEMV).  Untimed by bench.py's own clock."""
        np = self.np
        ok, res = True, None
        x = np.zeros(self.n)
        try:
            s.set_max_iter(steps)
            s.tolerance(0.0)
            res = s.solve(x)
        except Exception as e:             # noqa: BLE001
            self.log("solve-window run failed: %s" % e)
            ok = False
        if not self.all_ok(ok):
            return None
        secs = self.max_over_ranks(res["seconds_solve"])
        return {"iterations": res["iterations"], "seconds_solve": secs, "iterations_per_s": res["iterations"] / secs,
                "what": "one cgx_solve() of K iterations, the reference's window cg_main.cc:53-55 (setup + initial "
                        "GEMV + loop + gather of x + verification GEMV), max over ranks"}

    def dense_leg(self, s, warmup, steps):
        """K1 of the same solver on dense incompressible data: [median ms, samples, finite] of every rank, or None."""
        ok = True
        try:
            s.probe_fill_matrix_hash(0x5EEDC0DE, symmetric=True, diag=1.03 * 2.0 * math.sqrt(self.n / 3.0))
            s.init_source_term(1.0 / self.n)
        except Exception as e:             # noqa: BLE001
            self.log("dense-data leg: fill failed: %s" % e)
            ok = False
        if not self.all_ok(ok):
            return None
        out = self.run(s, warmup, steps)
        if out is None:
            return None
        _, r, _ = out
        return self.gather_rows([r["gemv_ms_median"], float(r["gemv_launches"]), 1.0 if math.isfinite(r["residual_prev"]) else 0.0])

    def measure(self):
        args, world, rank, n, pkg = self.args, self.world, self.rank, self.n, self.pkg
        if not self.use_comm:
            order = ["self"]
        elif args.transport == "auto":
            order = ["p2p-tag", "p2p", "p2p-sep", "rccl"]
        else:
            order = [args.transport]
        # Build every candidate transport that works on this node; with more than one, a short calibration run
        # (same workload, 60 iterations) decides which one carries the timed run.  All decisions are taken on
        # rank-reduced values, so every rank takes the same branch.
        solvers = {}
        for tname in order:
            cand = self.make_solver(tname)
            if cand is not None:
                solvers[tname] = cand
        # what the RCCL candidate spans (ncclCommCount on every rank), recorded while it exists: the calibration may hand the
        # timed run to the mailboxes, and the line must still say whether RCCL saw all N ranks (cg.cc:50-51)
        self.rccl_nranks = None
        if "rccl" in solvers:
            counts = self.gather_rows([float(solvers["rccl"].comm_info()["ranks_wired"])])
            self.rccl_nranks = int(min(c[0] for c in counts))
        self.state["stage"] = "pre-warm"
        for tname, cand in list(solvers.items()):
            if not self.prewarm(cand, tname):
                self.notes.append("%s dropped: pre-warm run failed" % tname)
                cand.close()
                del solvers[tname]
        calib = {}
        if len(solvers) > 1:
            self.state["stage"] = "transport calibration"
            for tname, cand in list(solvers.items()):
                c = self.run(cand, 30, 60)
                if c is None:
                    self.notes.append("%s dropped: calibration run failed" % tname)
                    cand.close()
                    del solvers[tname]
                else:
                    calib[tname] = self.max_over_ranks(c[0]) / 60 * 1e3
        self.state["stage"] = "timed run"
        out, transport, solver = None, None, None
        # auto: the tagged-word form is built, self-tested and calibrated for the record, but it does not carry the timed run
        # unless it is asked for by name (--transport p2p-tag): it rests on an 8-byte half of a 16-byte write-through store
        # arriving untorn over xGMI, which no run on more than one GPU has shown yet.
        eligible = [t for t in solvers if not (args.transport == "auto" and t == "p2p-tag" and len(solvers) > 1)]
        if "p2p-tag" in solvers and "p2p-tag" not in eligible:
            self.notes.append("p2p-tag calibrated for the record only (auto never selects it; --transport p2p-tag runs it)")
        for tname in sorted(eligible, key=lambda t: calib.get(t, 0.0)):
            out = self.run(solvers[tname], args.warmup, args.steps)
            if out is not None:
                transport, solver = tname, solvers[tname]
                break
            self.notes.append("%s dropped: timed run failed" % tname)
        if out is None:
            raise RuntimeError("no transport produced a result (%s)" % ("; ".join(self.notes) or "none could be built"))
        for tname, cand in solvers.items():
            if cand is not solver:
                cand.close()
        self.solver = solver
        elapsed, res, samples = out
        x_out = self.last_x                    # later runs on the solver (solve window, dense leg) replace self.last_x
        if res["iterations"] != args.warmup + args.steps:
            raise RuntimeError("the timed run stopped after %d of %d iterations: ms_per_step would not be per step"
                               % (res["iterations"], args.warmup + args.steps))
        elapsed = self.max_over_ranks(elapsed)

        # K1 statistics of every rank: [rows, samples, discarded, min, median, mean, max] (ms)
        starts, counts = pkg.partition(n, world)
        my_rows = counts[rank]
        k1_rows = self.gather_rows([my_rows, res["gemv_launches"], res["gemv_discarded"], res["gemv_ms_min"],
                                    res["gemv_ms_median"], res["gemv_ms_avg"], res["gemv_ms_max"]])
        us = sorted(float(v) for v in self.update_samples)
        upd_rows = self.gather_rows([float(len(us)), us[0] if us else 0.0, us[len(us) // 2] if us else 0.0, us[-1] if us else 0.0])
        dev_ms = self.max_over_ranks(res.get("steps_device_ms", 0.0))
        info = solver.comm_info()
        devices = self.gather_strings(info["device_id"])
        wired = self.gather_rows([info["ranks_wired"], info["rank_seen"]])
        plan = solver.gemv_plan()
        plan_keys = ("variant", "R", "U", "waves", "light", "split", "grid", "ncols")
        plans = [dict(zip(plan_keys, (int(v) for v in row))) for row in self.gather_rows([float(plan[k]) for k in plan_keys])]

        self.state["stage"] = "solve-window run"
        window = None if args.no_solve_window else self.solve_window(solver, args.steps)

        # Dense-data leg (last thing done with the solver: it overwrites the matrix).  generate_lap2d_matrix leaves 5 non-zeros
        # per row (cg.cc:178-186), the reference's GEMV is a general dense dgemv (cg.cc:101-102): the same K1 launches once more
        # on a row block in which every element is a different number (cgx_probe_fill_matrix_hash: symmetric, dominant
        # diagonal, so CG keeps running), same steps, same event timing.
        dense = None
        if not args.no_dense_check and self.profile_every:
            self.state["stage"] = "dense-data leg"
            dense = self.dense_leg(solver, args.warmup, args.steps)

        if rank != 0:
            return None
        dumped = dump_outputs(args.dump_outputs, x_out, res) if args.dump_outputs else None
        ms_per_step = elapsed / args.steps * 1e3
        per_rank = []
        for q, (rows_q, cnt, disc, mn, med, avg, mx) in enumerate(k1_rows):
            bytes_q = 8.0 * (rows_q * n + n + rows_q)          # A rows once + p + Ap
            per_rank.append({"rank": q, "rows": int(rows_q), "bytes_per_launch": bytes_q, "launches_timed": int(cnt),
                             "launches_discarded": int(disc), "min_ms": mn, "median_ms": med, "mean_ms": avg, "max_ms": mx,
                             "GBs": (bytes_q / (med * 1e-3) / 1e9) if med > 0 else None})
        timed_ranks = [r for r in per_rank if r["GBs"]]
        lim = min(timed_ranks, key=lambda r: r["GBs"]) if timed_ranks else None   # the rank furthest below the roofline
        slowest = max(timed_ranks, key=lambda r: r["median_ms"]) if timed_ranks else None
        roof = {
            "bound": "hbm", "achieved": None, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": None,
            "traffic": None,
            "traffic_source": "committed rocprofv3 --pmc pass of the same K1 form (config.k1_plan) at this n and shard count, "
                              "%s (FETCH_SIZE x2 + WRITE_SIZE per the guide's gfx950 correction); NOT a counter of this "
                              "run; null when no committed row matches the plan that ran" % TRAFFIC_FILE,
            "kernel": "k_gemv (K1, A.p of this rank's row block)",
            "timing": "HIP events bound to the K1 dispatch (kernel begin/end) on the library's stream, every %slaunch "
                      "of the timed region, median; the first launch after the sync is not sampled"
                      % ("" if self.profile_every == 1 else "%d-th " % self.profile_every),
        }
        if lim is not None:
            ok = lim["median_ms"] <= ms_per_step          # a kernel that runs once per step cannot outlast the step
            roof.update({
                "bytes_per_launch": lim["bytes_per_launch"], "median_launch_ms": lim["median_ms"],
                "avg_launch_ms": lim["mean_ms"], "min_launch_ms": lim["min_ms"], "max_launch_ms": lim["max_ms"],
                "launches_timed": lim["launches_timed"], "launches_discarded": lim["launches_discarded"],
                "rank": lim["rank"], "consistency": "ok" if ok else "violated",
            })
            roof["traffic"] = pmc_traffic(n, world, plans[lim["rank"]])
            if ok:
                roof["achieved"] = lim["GBs"]
                roof["frac"] = lim["GBs"] / HBM_PEAK_GBS
            else:
                roof["note"] = ("median_launch_ms exceeds ms_per_step: the K1 timing is not trustworthy for this run, "
                                "no fraction is reported")
        if dense is not None and lim is not None:
            dmed, dcnt, dfin = dense[lim["rank"]]
            if dmed > 0 and dfin:
                ratio = dmed / lim["median_ms"]
                roof["dense_random"] = {
                    "what": "the same K1 (same rank, same steps, same event timing) on a row block in which every element is a "
                            "different number in [-1, 1) (cgx_probe_fill_matrix_hash: counter-based hash, symmetric, dominant diagonal) "
                            "instead of generate_lap2d_matrix's 5 non-zeros per row; run after the timed region",
                    "median_launch_ms": dmed, "launches_timed": int(dcnt),
                    "achieved": lim["bytes_per_launch"] / (dmed * 1e-3) / 1e9, "frac": lim["bytes_per_launch"] / (dmed * 1e-3) / 1e9 / HBM_PEAK_GBS,
                    "time_ratio_to_generated_matrix": ratio,
                }
                if abs(ratio - 1.0) > 0.01:
                    roof["dense_random"]["note"] = ("K1 on dense data differs from K1 on the generated matrix by more than 1 % on this box: "
                                                    "the headline fraction is data dependent here")
        line = base_line(args, world, n)
        rows0 = counts[0]
        line.update({"value": args.steps / elapsed, "ms_per_step": ms_per_step})
        line["config"].update({
            "rows_per_gpu": rows0,
            "collectives": {"self": "none",
                            "rccl": "1 x ncclAllGather per iteration ([Ap slice | p.Ap partials])",
                            "p2p-tag": "1 exchange per iteration over IPC/xGMI mailboxes, folded into K3, tagged 8-byte words, no flags "
                                       "or fences ([Ap slice | p.Ap partial per chunk])",
                            "p2p": "1 exchange per iteration over IPC/xGMI mailboxes, folded into K3 ([Ap slice | p.Ap])",
                            "p2p-sep": "1 mailbox all-gather kernel per iteration over IPC/xGMI ([Ap slice | p.Ap])"}[transport],
            "transport": transport,
            "transport_calibration_ms_per_iteration": calib or None,
            "transport_notes": self.notes or None,
            "k1_variant": args.variant,
            "prewarm_iterations": self.prewarm_iterations.get(transport),   # untimed, before the W warm-up steps
            # what the transports really span (from the transports, not from the flags)
            "process_group_ranks": self.dist.get_world_size() if self.dist is not None else 1,
            # ncclCommCount of the library's RCCL communicator (min over ranks): of the transport that ran, or of the RCCL
            # candidate of the calibration when the mailboxes carried the timed run; None if no RCCL communicator was built
            "rccl_nranks": int(wired[0][0]) if transport == "rccl" else self.rccl_nranks,
            "k1_plan": plans if world > 1 else plans[0],     # the K1 form the library ran on every rank (cgx_get_gemv_plan)
            "transport_ranks_wired": [int(w[0]) for w in wired],
            "ranks_seen": len(k1_rows),                                            # ranks whose results were compared bit for bit
            "distinct_gpus": len(set(devices)), "gpu_pci_ids": devices,
        })
        line["roofline"] = roof
        if world > 1:
            line["k1_per_rank"] = per_rank
            line["k1_slowest_rank"] = slowest["rank"] if slowest else None
        if any(u[0] > 0 for u in upd_rows):
            # the update kernel of the same iterations whose K1 was timed: K3, or (p2p) K3 with the exchange inside, whose
            # duration holds the bounded wait for every peer's chunks -- what the exchange costs each rank (cg.cc:106,135-136)
            line["update_kernel"] = {
                "kernel": {"p2p": "k_update_xr_p2p (K3 with the exchange inside)",
                           "p2p-tag": "k_update_xr_p2p_tagged (K3 with the exchange inside, tagged words)"}.get(transport, "k_update_xr (K3)"),
                "timing": "HIP events bound to the dispatch, the launches whose K1 was timed",
                "per_rank": [{"rank": q, "launches_timed": int(u[0]), "min_ms": u[1], "median_ms": u[2], "max_ms": u[3]}
                             for q, u in enumerate(upd_rows)],
            }
        if dev_ms > 0:
            # the same K steps on the device's own clock (markers in front of the first and behind the last kernel of
            # the timed call, max over ranks): what is left to ms_per_step is launch latency and the final synchronise
            line["device_window_ms_per_step"] = dev_ms / args.steps
        line["aggregate_gemv_GBs"] = sum(r["GBs"] for r in timed_ranks) if timed_ranks else None
        line["whole_iteration_GBs_per_gpu"] = 8.0 * (rows0 * n + n + 14 * rows0) / (elapsed / args.steps) / 1e9
        if 0 < len(samples) <= 64:
            line["k1_samples_ms"] = [round(float(v), 5) for v in samples]      # rank 0's launches, launch order
        line["residual_after_run"] = res["residual_prev"]
        if dumped is not None:
            line["dumped_outputs"] = dumped
        line["iterations_done"] = res["iterations"]
        if window is not None:
            line["solve_window_iterations_per_s"] = window["iterations_per_s"]
            line["solve_window"] = window
            self.gpu_work_s += window["seconds_solve"]
            self.gpu_iterations += window["iterations"]
        # for a reader of a GPU-utilisation sampler beside this line: how much device work the process did in all (the
        # rest of a 1-GPU run's wall time is the CPU baseline, which keeps the GPU idle)
        line["gpu_work"] = {"seconds_in_timed_loops": self.gpu_work_s, "cg_iterations_on_device": self.gpu_iterations}
        # From here on only extras are added (live counters, CPU baseline): the measurement is complete.  A snapshot goes to
        # the watchdog, so that an extra that hangs costs the extras, never the line.
        self.state["line_snapshot"] = json.dumps(line)
        if world == 1 and transport == "self" and not args.no_live_pmc and lim is not None:
            # the traffic of THIS box, by counters, instead of the committed constant: two rocprofv3 --pmc child passes of the
            # same workload (after the timed region; the parent keeps its own matrix, the child builds another)
            self.state["stage"] = "live PMC passes"
            live, note = live_pmc_traffic(args, n)
            roof["traffic_committed"] = roof["traffic"]
            if live is not None:
                roof["traffic"] = live
                roof["traffic_over_algorithmic"] = live / lim["bytes_per_launch"]
                roof["traffic_source"] = ("LIVE: two rocprofv3 --pmc child passes of this program on this box, FETCH_SIZE then WRITE_SIZE, "
                                          "--kernel-trace only (%s); read bytes = FETCH_SIZE x 1024 x 2 (the guide's gfx950 correction), "
                                          "WRITE_SIZE x 1024 exact; traffic_committed = the row of %s for the same K1 plan" % (note, TRAFFIC_FILE))
            else:
                roof["traffic_live_note"] = note
        if world == 1 and transport == "self" and not args.no_reference_sizes:
            self.state["stage"] = "reference sizes"
            try:
                line["reference_sizes"] = reference_sizes(pkg, self.torch)
            except Exception as e:                 # noqa: BLE001 -- an extra must never cost the line
                line["reference_sizes"] = {"error": str(e)[:200]}
        if not args.no_cpu_baseline:
            # rank 0 only, after the timed region and outside every bracket; the other ranks wait at the teardown barrier
            self.state["stage"] = "cpu baseline"
            if args.test_hang == "extra:cpu baseline":   # test hook: an extra that never comes back
                time.sleep(3600)
            line["cpu_baseline"] = cpu_baseline(n, args.cpu_baseline_iters)
        return line

    def teardown(self):
        if getattr(self, "solver", None) is not None:
            self.solver.close()
        if self.dist is not None:
            self.dist.barrier()
            self.dist.destroy_process_group()


def free_port():
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


# children with a process group of their own, for the watchdog / SIGTERM paths to stop: the launcher child of self_launch
# ("proc") and the rocprofv3 pass of live_pmc_traffic that is running right now ("extra")
LAUNCHED = {"proc": None, "extra": None}


def stop_group(proc):
    """End a child that was started with start_new_session=True, and everything under it."""
    if proc is None or proc.poll() is not None:
        return
    for sig, wait in ((signal.SIGTERM, 10.0), (signal.SIGKILL, 5.0)):
        try:
            os.killpg(proc.pid, sig)
        except (ProcessLookupError, PermissionError):
            return
        try:
            proc.wait(wait)
            return
        except subprocess.TimeoutExpired:
            pass


def stop_launched():
    """End the launcher child and every rank under it, and a counter pass in flight, if there is one."""
    stop_group(LAUNCHED["proc"])
    stop_group(LAUNCHED["extra"])


def self_launch(args, emit_raw, failure_line, state):
    """`python bench.py --gpus N` with no launcher around it (RANK / WORLD_SIZE unset): this process becomes the launcher.
    It starts `python -m torch.distributed.run --nproc-per-node N bench.py <same arguments>` as a FRESH CHILD process --
    before torch is imported or HIP is touched here, and never by exec -- relays the one JSON line rank 0 prints, passes
    stderr through, and leaves with the child's exit code.  (The reference gets its ranks from `srun -n P`,
    code/MPI/cg_main.cc:15-20 and cg.run:15-19; the GPU box has no such launcher by itself.)  Returns the exit code."""
    state["stage"] = "self-launch of %d ranks" % args.gpus
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    env.setdefault("OMP_NUM_THREADS", "1")
    print("bench.py: starting %d ranks: %s" % (args.gpus, " ".join(cmd)), file=sys.stderr, flush=True)
    proc = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=None, env=env, start_new_session=True)
    LAUNCHED["proc"] = proc
    relayed = False
    for raw in proc.stdout:                       # ends when every holder of the pipe has closed it
        text = raw.decode(errors="replace").strip()
        if not relayed and text.startswith("{"):
            try:
                ok = "metric" in json.loads(text)
            except ValueError:
                ok = False
            if ok:
                relayed = emit_raw(text)
                continue
        if text:
            print(text, file=sys.stderr, flush=True)
    rc = proc.wait()
    if not relayed:
        emit_raw(json.dumps(failure_line("launch", "the %d ranks started by bench.py ended with exit code %d without a result "
                                                   "line (see stderr)" % (args.gpus, rc))))
        rc = rc or 1
    return rc


def main():
    args = parse_args()
    # stdout carries the ONE JSON line and nothing else: whatever the libraries print on fd 1 while the run is
    # going (RCCL's version banner, for one) is sent to stderr instead.
    sys.stdout.flush()
    json_fd = os.dup(1)
    os.dup2(2, 1)
    # cross-process device memory (the mailboxes, RCCL's own buffers) needs dmabuf IPC on this driver; keep the setting
    # the image exports even if a launcher scrubbed the environment.  Before torch / HIP are loaded.
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    state = {"stage": "start", "printed": False}
    lock = threading.Lock()

    def emit_raw(text):
        """Rank 0 prints exactly one line, whoever gets here first (main thread, watchdog or signal handler)."""
        with lock:
            if rank != 0 or state["printed"]:
                return False
            state["printed"] = True
            os.write(json_fd, (text + "\n").encode())
            return True

    def emit(line):
        emit_raw(json.dumps(line))

    def failure_line(kind, message):
        line = base_line(args, max(world, args.gpus), problem_size(args, max(world, args.gpus)))
        line["error"] = {"kind": kind, "stage": state["stage"], "message": str(message)[:2000]}
        return line

    def on_watchdog():
        printed = state["printed"]
        stop_launched()
        if state.get("line_snapshot") and not printed:
            # the timed result exists; what hung is an extra (live PMC passes, CPU baseline): print the measurement without it
            snap = json.loads(state["line_snapshot"])
            snap["watchdog_note"] = "stage '%s' did not finish within the %.0f s watchdog; the line is complete up to it" % (state["stage"], args.watchdog)
            emit(snap)
            print("bench.py rank %d: watchdog expired in stage '%s' (line printed without it)" % (rank, state["stage"]), file=sys.stderr, flush=True)
            os._exit(0)
        emit(failure_line("watchdog", "no result after %.0f s" % args.watchdog))
        print("bench.py rank %d: watchdog expired in stage '%s'" % (rank, state["stage"]), file=sys.stderr, flush=True)
        os._exit(0 if printed else 3)

    def wait_for_sigterm():
        # SIGTERM is what the launcher sends when another rank died.  A Python-level handler would only run once the
        # main thread is back from whatever C call it is blocked in, so a dedicated thread waits for the signal.
        signum = signal.sigwait({signal.SIGTERM})
        stop_launched()
        emit(failure_line("signal", "received signal %d (the launcher stops this rank: another rank failed?)" % signum))
        os._exit(4)

    signal.pthread_sigmask(signal.SIG_BLOCK, {signal.SIGTERM})   # before any thread exists: every thread inherits the mask
    threading.Thread(target=wait_for_sigterm, daemon=True, name="bench-sigterm").start()
    launcher = args.gpus > 1 and "RANK" not in os.environ and "WORLD_SIZE" not in os.environ
    # the ranks run their own watchdog of args.watchdog seconds and print their own failure line; the launching parent's is
    # the backstop behind it
    dog = threading.Timer(args.watchdog + (60.0 if launcher else 0.0), on_watchdog)
    dog.daemon = True
    dog.start()

    if launcher:
        rc = 1
        try:
            rc = self_launch(args, emit_raw, failure_line, state)
        except BaseException as e:           # noqa: BLE001 -- the line must still come out
            traceback.print_exc(file=sys.stderr)
            stop_launched()
            emit(failure_line(type(e).__name__, e))
        sys.stderr.flush()
        os._exit(rc)
    if world != args.gpus:
        args.gpus = world

    b = Bench(args, world, rank, local_rank, state)
    rc = 0
    try:
        b.init()
        line = b.measure()
        if rank == 0:
            emit(line)
        state["stage"] = "teardown"
        b.teardown()
    except BaseException as e:               # noqa: BLE001 -- rank 0 must still print its line
        traceback.print_exc(file=sys.stderr)
        emit(failure_line(type(e).__name__, e))
        rc = 1
    sys.stderr.flush()
    # Abandoned helper threads (a wire-up stage that timed out) must not keep the process alive, hence os._exit on
    # every path but the clean one; the clean one leaves normally so that a profiler's exit handlers still run.
    if rc != 0 or any(t.name.startswith("bench-") and t.name != "bench-sigterm" for t in threading.enumerate()):
        os._exit(rc)
    sys.exit(0)


if __name__ == "__main__":
    main()
