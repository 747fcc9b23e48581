"""Worker for tests/test_gpu_jacobi.py: one OS process per rank, all on ONE GPU, over the CGX_COMM_P2P mailboxes.  Every rank
solves the generated matrix (diagonal 4) plainly and with Jacobi on the same context; rank 0 writes "same bits" if x and the
reported numbers agree bit for bit on every rank.  argv: n max_iter out tagged(0|1) [matrix]
matrix "scaled" (tests/test_gpu_jacobi_scaled.py): L = the generated matrix, s_i = 2**e_i seeded alike on every rank; plain CG on
(L, b~) and Jacobi on (S L S, S b~) on the same context; "same bits" only if s * x equals x~ bit for bit on every rank."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402


def _scaled_runs(s, n, iters, world):
    """(ok, what to report): plain on L, Jacobi on S L S, both tol = 0 and `iters` iterations from x0 = 0."""
    O = g.load_oracle()
    L = O.generate_lap2d(n)
    sc = np.ldexp(1.0, np.random.default_rng(20261016).integers(-8, 9, n))
    bt = O.init_source_term(n)
    runs, plan_ok = [], True
    for kind, A, b in ((None, L, bt), ("jacobi", (sc[:, None] * L) * sc[None, :], sc * bt)):
        s.set_matrix_dense(A)
        plan_ok = plan_ok and s.gemv_plan()["variant"] == 1 and s.nranks == world == 3   # no assert: the peers would wait
        s.set_preconditioner(kind)   # every rank, the same value
        s.set_max_iter(iters)
        s.tolerance(0.0)
        s.set_source_term(b)
        x = np.zeros(n)
        dist.barrier()
        res = s.solve(x)
        nb = np.linalg.norm(b)
        true_rel = float(np.linalg.norm(A @ x - b) / nb)
        # what an fp64 evaluation of A x - b may be off by (rows of at most 5 entries): 7 eps (|A||x| + |b|) per row
        floor = float(np.linalg.norm(7 * np.finfo(np.float64).eps * (np.abs(A) @ np.abs(x) + np.abs(b))) / nb)
        runs.append((x, res["iterations"], res["rel_residual"], true_rel, floor))
    (xt, kt, _, _, _), (xj, kj, rel, true_rel, floor) = runs
    ok = plan_ok and kt == kj == iters and np.array_equal((sc * xj).view(np.uint64), xt.view(np.uint64))
    ok = ok and abs(rel - true_rel) <= 1e-9 * true_rel + 2 * floor
    return ok, [r[1:] for r in runs]


def _lap2d_runs(s, n, iters):
    s.generate_lap2d_matrix(n)
    keys = ("iterations", "converged", "residual_prev", "residual_last", "rel_residual", "x_norm")
    runs = []
    for kind, tol in ((None, 0.0), ("jacobi", 0.0), (None, 1e-3), ("jacobi", 1e-3)):
        s.set_preconditioner(kind)   # every rank, the same value
        s.set_max_iter(iters if tol == 0.0 else 4 * n)
        s.tolerance(tol)
        s.init_source_term(1.0 / n)
        x = np.zeros(n)
        dist.barrier()
        res = s.solve(x)
        runs.append((x, [float(res[k]) for k in keys]))
    ok = all(np.array_equal(runs[i][0].view(np.uint64), runs[i + 1][0].view(np.uint64)) and runs[i][1] == runs[i + 1][1]
             for i in (0, 2))
    ok = ok and runs[3][1][1] == 1.0   # the tolerance run converged
    return ok, [r[1] for r in runs]


def main():
    n, iters, out, tagged = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4] == "1"
    matrix = sys.argv[5] if len(sys.argv) > 5 else "lap2d"
    assert matrix in ("lap2d", "scaled"), matrix
    dist.init_process_group(backend="gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    assert torch.cuda.is_available()
    pkg = g.load_package()
    s = pkg.CGSolver(comm_mode=pkg.COMM_P2P, nranks=world, rank=rank, device=0, p2p_timeout_ms=20000, p2p_tagged=tagged)
    mine = torch.tensor(list(s.p2p_export()), dtype=torch.uint8)
    allh = [torch.zeros_like(mine) for _ in range(world)]
    dist.all_gather(allh, mine)
    s.p2p_import(b"".join(bytes(t.tolist()) for t in allh))
    dist.barrier()
    assert s.p2p_selftest(16)
    dist.barrier()
    ok, report = _lap2d_runs(s, n, iters) if matrix == "lap2d" else _scaled_runs(s, n, iters, world)
    flags = [torch.zeros(1) for _ in range(world)]
    dist.all_gather(flags, torch.tensor([1.0 if ok else 0.0]))
    s.close()
    dist.barrier()
    dist.destroy_process_group()
    if rank == 0:
        with open(out, "w") as f:
            f.write("same bits" if all(float(t) == 1.0 for t in flags) else "differ: %r" % (report,))


if __name__ == "__main__":
    main()
