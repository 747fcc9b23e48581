"""The Jacobi preconditioner on the GPU (include/cgx.h cgx_set_preconditioner).

1. Bit identity where the mathematics demands it.  With a diagonal that is one power of two c (generate_lap2d has 4; the symmetric
   hash matrix takes diag = 2**k above n, which keeps it diagonally dominant: its off-diagonal entries lie in [-1, 1)), z = r / c,
   rho = r.r / c and p_Jacobi = p / c are exact scalings, alpha_Jacobi = c alpha exactly, and x, r and every reported number must
   be the plain run's bit for bit -- through variant 6, 10821 and a v = 2 shape, with and without a tolerance, on loopback shards,
   on P2P processes (tests/p2p_jacobi_worker.py), through the CLI on the RCCL transport, and from x0 != 0.  (The bound of the alpha
   safeguard scales differently, so the problems are kept far from breakdown.)
2. A non-uniform diagonal: A = S L S (L = lap2d, s_i spread over [1, 100]) against a numpy longdouble PCG of the same recurrence.
3. What it is for: on that matrix Jacobi needs about as many iterations as plain CG on L, plain CG on S L S many times more.
4. Refusals and state.  5. The CLI switch."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "conjugate-gradient_amd", "cgsolver")
SEED = 0x7AC0B1
BAD_ARG, UNSUPPORTED = 1, 7


def _run(pkg, n, variant, jacobi, iters, tol, matrix="lap2d", comm=None, nranks=1, x0=None, **kw):
    cm = pkg.COMM_SELF if comm is None else comm
    with pkg.CGSolver(comm_mode=cm, nranks=nranks, gemv_variant=variant, **kw) as s:
        s.generate_lap2d_matrix(n)
        if matrix == "hash":
            s.probe_fill_matrix_hash(SEED, symmetric=True, diag=float(2 ** int(np.ceil(np.log2(n + 1)))))
        if jacobi:
            s.set_preconditioner("jacobi")
        assert s.preconditioner == ("jacobi" if jacobi else None)
        s.set_max_iter(iters)
        s.tolerance(tol)
        s.init_source_term(1.0 / n)
        plan = s.gemv_plan()
        x = np.zeros(n) if x0 is None else np.array(x0, dtype=np.float64)
        if x0 is None:
            res = s.solve(x)
        else:
            s.solve_begin(x)
            s.solve_steps(iters)
            res = s.solve_end(x)
    return x, res, plan


def _same_bits(a, b):
    (xa, ra, _), (xb, rb, _) = a, b
    assert np.array_equal(xa.view(np.uint64), xb.view(np.uint64)), np.max(np.abs(xa - xb))
    for key in ("iterations", "converged", "residual_prev", "residual_last", "rel_residual", "x_norm"):
        assert ra[key] == rb[key], (key, ra[key], rb[key])


# ---- 1. bit identity ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,n,want", [(-1, 16900, 6), (10821, 4096, 1), (20421, 4096, 2)])
@pytest.mark.parametrize("matrix", ["lap2d", "hash"])
@pytest.mark.parametrize("tol", [0.0, "loose"])
def test_power_of_two_diagonal_gives_the_plain_bits(gpu_pkg, variant, n, want, matrix, tol):
    iters = 40
    if tol == "loose":   # converges inside max_iter: the break and its iteration are compared too
        tol = 1e-3 if matrix == "lap2d" else 1e-9
        iters = 2000
    plain = _run(gpu_pkg, n, variant, False, iters, tol, matrix)
    pcg = _run(gpu_pkg, n, variant, True, iters, tol, matrix)
    assert plain[2]["variant"] == pcg[2]["variant"] == want, (plain[2], pcg[2])
    if tol > 0:
        assert pcg[1]["converged"] == 1 and 0 < pcg[1]["iterations"] < iters, pcg[1]
    _same_bits(plain, pcg)


@pytest.mark.parametrize("n,p", [(4096, 2), (3001, 3), (2048, 8), (5, 8)])   # (5, 8): every shard but the last is empty
def test_loopback_shards_give_the_plain_bits(gpu_pkg, n, p):
    iters = 3 if n < 16 else 60
    plain = _run(gpu_pkg, n, 0, False, iters, 0.0, comm=gpu_pkg.COMM_LOOPBACK, nranks=p)
    pcg = _run(gpu_pkg, n, 0, True, iters, 0.0, comm=gpu_pkg.COMM_LOOPBACK, nranks=p)
    _same_bits(plain, pcg)


def test_nonzero_initial_guess_gives_the_plain_bits(gpu_pkg):
    n = 4096
    x0 = np.random.default_rng(7).standard_normal(n)
    plain = _run(gpu_pkg, n, 10821, False, 50, 0.0, x0=x0)
    pcg = _run(gpu_pkg, n, 10821, True, 50, 0.0, x0=x0)
    _same_bits(plain, pcg)


@pytest.mark.parametrize("tagged,port", [(0, 29781), (1, 29782)])
def test_p2p_processes_give_the_plain_bits(tmp_path, tagged, port):
    out = tmp_path / "p2p_jacobi.json"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "3", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "p2p_jacobi_worker.py"), "3000", "80", str(out), str(tagged)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=420, env=dict(os.environ, OMP_NUM_THREADS="1", MASTER_ADDR="127.0.0.1"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert open(out).read().strip() == "same bits", open(out).read()


def _loop_bodies(stderr):
    m = re.search(r"cgsolver stats: .*", stderr)
    assert m, stderr[-2000:]
    return m.group(0), int(re.search(r"loop_bodies=(\d+)", m.group(0)).group(1))


@pytest.fixture(scope="module")
def fake_rccl_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("fake_rccl_jacobi")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-w", "-O2", "-std=c++17", "-fPIC", "-shared", "-I/opt/rocm/include",
                           os.path.join(ROOT, "tests", "fake_rccl", "fake_rccl.cc"), "-o", str(d / "librccl.so.1"),
                           "-Wl,-soname,librccl.so.1"], timeout=600)
    return str(d)


def test_cli_rccl_transport_gives_the_plain_loop(gpu_pkg, fake_rccl_dir, tmp_path):
    env = dict(os.environ, LD_LIBRARY_PATH=fake_rccl_dir + os.pathsep + os.environ.get("LD_LIBRARY_PATH", ""))
    base = ["2048", str(tmp_path / "out"), "--gpus", "2", "--same-device", "--transport", "rccl", "--stats"]
    rp = subprocess.run([EXE] + base, capture_output=True, text=True, timeout=300, env=env)
    rj = subprocess.run([EXE] + base + ["--jacobi"], capture_output=True, text=True, timeout=300, env=env)
    assert rp.returncode == 0 and rj.returncode == 0, rp.stderr[-2000:] + rj.stderr[-2000:]
    assert "fake_rccl: rank 1 of 2 wired" in rj.stderr
    lp, kp = _loop_bodies(rp.stderr)
    lj, kj = _loop_bodies(rj.stderr)
    assert "precond=" not in lp and lj.endswith("precond=jacobi"), (lp, lj)
    assert kp == kj and kp > 10, (lp, lj)


# ---- 2. and 3. S L S ----------------------------------------------------------------------------------------------------------
N_SLS = 1024


def _sls(oracle, n=N_SLS):
    L = oracle.generate_lap2d(n)
    s = np.geomspace(1.0, 100.0, n)[np.random.default_rng(20261015).permutation(n)]
    return L, (s[:, None] * L) * s[None, :]


def _pcg_longdouble(A, b, iters, tol=0.0):
    """The library's recurrence in np.longdouble; returns (x, iterations as the library counts them)."""
    A = A.astype(np.longdouble)
    b = b.astype(np.longdouble)
    dinv = 1 / np.diag(A)
    x = np.zeros_like(b)
    r = b.copy()
    z = dinv * r
    p = z.copy()
    rho = r @ z
    prev = np.sqrt(r @ r)
    for k in range(iters):
        Ap = A @ p
        alpha = rho / (p @ Ap)
        x += alpha * p
        r -= alpha * Ap
        if np.sqrt(r @ r) < tol:
            _pcg_longdouble.residual_prev = float(prev)   # sqrt(r.r) before the last update: what residual_prev reports
            return x.astype(np.float64), k
        prev = np.sqrt(r @ r)
        z = dinv * r
        rn = r @ z
        p = z + (rn / rho) * p
        rho = rn
    return x.astype(np.float64), iters


# Derived on the CPU with _pcg_longdouble (and a float64 restatement in 4 summation orders) for n = 1024, b = init_source_term,
# tol = 1e-6 ||b|| = 0.228466...: plain CG on L stops at iteration 90, Jacobi on S L S at 103 (its last residual 0.22790 against
# tol 0.22847: far from a rounding tie), plain CG on S L S at 2480 (2.4 n; in float64 it does not converge within n).
K_PLAIN_L, K_JACOBI_SLS, K_PLAIN_SLS = 90, 103, 2480
MARGIN = K_JACOBI_SLS - K_PLAIN_L   # 13: what Jacobi on S L S needs beyond plain CG on L, from the same reference
# Fixed-k accuracy: float64 PCG against the longdouble one, worst over k = 20, 60, 100, 150 and 4 summation orders:
# 6.1e-16 relative.  The bound below leaves five orders of magnitude for the GPU's summation order.
REL_BOUND = 1e-10


def _tol(oracle):
    return 1e-6 * float(np.linalg.norm(oracle.init_source_term(N_SLS)))


def _solve_dense(pkg, A, jacobi, iters, tol, variant=0):
    n = A.shape[0]
    with pkg.CGSolver(gemv_variant=variant) as s:
        s.set_preconditioner("jacobi" if jacobi else None)
        s.set_matrix_dense(A)
        s.set_max_iter(iters)
        s.tolerance(tol)
        s.init_source_term(1.0 / n)
        x = np.zeros(n)
        res = s.solve(x)
    return x, res


@pytest.mark.parametrize("variant", [0, -1, 20421])
def test_nonuniform_diagonal_against_longdouble(gpu_pkg, oracle, variant):
    L, A = _sls(oracle)
    b = oracle.init_source_term(N_SLS)
    k = 60
    x, res = _solve_dense(gpu_pkg, A, True, k, 0.0, variant)
    xr, _ = _pcg_longdouble(A, b, k)
    assert res["iterations"] == k
    err = np.linalg.norm(x - xr) / np.linalg.norm(xr)
    assert err <= REL_BOUND, err
    tol = _tol(oracle)
    x, res = _solve_dense(gpu_pkg, A, True, N_SLS, tol, variant)
    _, kref = _pcg_longdouble(A, b, N_SLS, tol)
    assert kref == K_JACOBI_SLS
    assert res["converged"] == 1 and res["iterations"] == kref, res
    # residual_prev / residual_last: sqrt(r.r) before and after the last update (as printed by the reference), not sqrt(r.z)
    assert res["residual_last"] < tol <= res["residual_prev"], res
    assert abs(res["residual_prev"] - _pcg_longdouble.residual_prev) <= 1e-9 * _pcg_longdouble.residual_prev, res


def test_jacobi_does_its_job(gpu_pkg, oracle):
    L, A = _sls(oracle)
    tol = _tol(oracle)
    _, rl = _solve_dense(gpu_pkg, L, False, N_SLS, tol)
    _, rj = _solve_dense(gpu_pkg, A, True, N_SLS, tol)
    _, rp = _solve_dense(gpu_pkg, A, False, N_SLS, tol)
    assert rl["converged"] == 1 and rl["iterations"] == K_PLAIN_L, rl
    assert rj["converged"] == 1 and rj["iterations"] <= rl["iterations"] + MARGIN, (rj, rl)
    assert rp["converged"] == 0 or rp["iterations"] >= 5 * rj["iterations"], rp


# ---- 4. refusals and state ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [0.0, -2.0, float("nan")])
def test_bad_diagonal_is_refused_on_every_shard_and_the_context_stays_usable(gpu_pkg, oracle, bad):
    n, row = 999, 700   # row 700 lies on the last of 3 loopback shards
    A = oracle.generate_lap2d(n)
    A[row, row] = bad
    with gpu_pkg.CGSolver(comm_mode=gpu_pkg.COMM_LOOPBACK, nranks=3) as s:
        s.set_matrix_dense(A)
        s.init_source_term(1.0 / n)
        s.set_max_iter(20)
        s.set_preconditioner("jacobi")
        with pytest.raises(gpu_pkg.CgxError) as e:
            s.solve(np.zeros(n))
        assert e.value.status == BAD_ARG and "row %d" % row in str(e.value), str(e.value)
        with pytest.raises(gpu_pkg.CgxError) as e:          # still refused: the check runs again
            s.solve(np.zeros(n))
        assert e.value.status == BAD_ARG
        s.set_preconditioner(None)
        A[row, row] = 4.0
        s.set_matrix_dense(A)
        s.init_source_term(1.0 / n)
        s.set_max_iter(20)
        x = np.zeros(n)
        assert s.solve(x)["iterations"] == 20
        s.set_preconditioner("jacobi")                      # a new matrix is extracted again
        assert s.solve(np.zeros(n))["iterations"] == 20


def test_unsupported_combinations(gpu_pkg, monkeypatch):
    monkeypatch.delenv("CGX_RESIDENT", raising=False)
    n = 2048
    with gpu_pkg.CGSolver() as s:
        s.generate_lap2d_matrix(n)
        s.init_source_term(1.0 / n)
        s.set_preconditioner("jacobi")
        with pytest.raises(gpu_pkg.CgxError) as e:
            s.solve_multi(np.ones((2, n)))
        assert e.value.status == UNSUPPORTED
    with gpu_pkg.CGSolver(matrix_format=gpu_pkg.MATRIX_BANDED) as s:
        s.generate_lap2d_matrix(n)
        s.init_source_term(1.0 / n)
        s.set_preconditioner("jacobi")
        with pytest.raises(gpu_pkg.CgxError) as e:
            s.solve(np.zeros(n))
        assert e.value.status == UNSUPPORTED
    for variant in (40000, 50000):
        with gpu_pkg.CGSolver(gemv_variant=variant) as s:
            s.generate_lap2d_matrix(n)
            s.init_source_term(1.0 / n)
            s.set_preconditioner("jacobi")
            with pytest.raises(gpu_pkg.CgxError) as e:
                s.solve(np.zeros(n))
            assert e.value.status == UNSUPPORTED


def test_setting_is_refused_inside_a_solve_and_for_an_unknown_kind(gpu_pkg):
    n = 1024
    with gpu_pkg.CGSolver(gemv_variant=-1) as s:
        s.generate_lap2d_matrix(n)
        s.init_source_term(1.0 / n)
        L = gpu_pkg.cgx.lib()
        assert L.cgx_set_preconditioner(s._h, 7) == BAD_ARG
        s.solve_begin(np.zeros(n))
        assert L.cgx_set_preconditioner(s._h, 1) == BAD_ARG
        s.solve_steps(5)
        s.solve_end(np.zeros(n))
        assert s.preconditioner is None


def test_persistent_choice_is_parked_and_comes_back(gpu_pkg, monkeypatch):
    monkeypatch.delenv("CGX_RESIDENT", raising=False)
    n = 2048
    with gpu_pkg.CGSolver() as s:
        s.generate_lap2d_matrix(n)
        s.init_source_term(1.0 / n)
        s.set_max_iter(100)
        assert s.gemv_plan()["variant"] == 4
        s.set_preconditioner("jacobi")
        assert s.gemv_plan()["variant"] == 1                 # per-launch while Jacobi is on
        rj = s.solve(np.zeros(n))
        s.generate_lap2d_matrix(n)                           # a new problem keeps the setting and the per-launch path
        s.init_source_term(1.0 / n)
        s.set_max_iter(100)
        assert s.gemv_plan()["variant"] == 1
        s.set_preconditioner(None)
        assert s.gemv_plan()["variant"] == 4
        x_after = np.zeros(n)
        r_after = s.solve(x_after)
    with gpu_pkg.CGSolver() as s:
        s.generate_lap2d_matrix(n)
        s.init_source_term(1.0 / n)
        s.set_max_iter(100)
        x_fresh = np.zeros(n)
        r_fresh = s.solve(x_fresh)
    assert rj["iterations"] == r_after["iterations"] == 100
    _same_bits((x_after, r_after, None), (x_fresh, r_fresh, None))


def test_cleared_per_launch_solve_matches_a_fresh_context(gpu_pkg):
    n = 4096
    with gpu_pkg.CGSolver(gemv_variant=10821) as s:
        s.generate_lap2d_matrix(n)
        s.probe_fill_matrix_hash(SEED, symmetric=True, diag=8192.0)
        s.init_source_term(1.0 / n)
        s.set_max_iter(30)
        s.tolerance(0.0)
        s.set_preconditioner("jacobi")
        s.solve(np.zeros(n))
        s.set_preconditioner(None)
        x1 = np.zeros(n)
        r1 = s.solve(x1)
    x2, r2, _ = _run(gpu_pkg, n, 10821, False, 30, 0.0, "hash")
    _same_bits((x1, r1, None), (x2, r2, None))


# ---- 5. CLI -------------------------------------------------------------------------------------------------------------------
def test_cli_jacobi_switch(gpu_pkg, tmp_path):
    out = tmp_path / "out"
    rj = subprocess.run([EXE, "--jacobi", "--stats", "1024", str(out)], capture_output=True, text=True, timeout=300)
    rp = subprocess.run([EXE, "--stats", "1024", str(out)], capture_output=True, text=True, timeout=300,
                        env=dict(os.environ, CGX_RESIDENT="0"))
    assert rj.returncode == 0 and rp.returncode == 0, rj.stderr[-2000:] + rp.stderr[-2000:]
    lines = open(out).read().split()
    assert len(lines) == 2 and all(re.fullmatch(r"1024,1,[0-9.eE+-]+", ln) for ln in lines), lines
    lj, kj = _loop_bodies(rj.stderr)
    lp, kp = _loop_bodies(rp.stderr)
    assert " precond=jacobi" in lj and " loop=per-launch" in lj, lj
    assert "precond=" not in lp, lp
    assert kj == kp, (lj, lp)
    usage = subprocess.run([EXE], capture_output=True, text=True, timeout=60)
    assert "--jacobi" in usage.stderr
