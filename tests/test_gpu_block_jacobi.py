"""Block Jacobi on the GPU (include/cgx.h cgx_set_preconditioner_block).

The reference is tests/block_jacobi_reference.py: the library's PCG recurrence with z = D_b^-1 r in np.longdouble, the block
inverses formed in longdouble too.

1. The inverse alone, through cgx_probe_get_precond_blocks: symmetric bit for bit, zero outside its blocks, and
   max |W_blk D_blk - I| <= 4 m 2^-52 kappa_2(D_blk) evaluated in longdouble (fp64 Cholesky and Gauss-Jordan measure at most
   0.30 m 2^-52 kappa on these cases: the bar leaves a factor 13).
2. Fixed iterations (k = 12 and 40) against the longdouble PCG, ||x - x_ref|| <= 1e-10 ||x_ref|| (tests/test_gpu_jacobi.py's
   REL_BOUND; three fp64 ways of forming the inverse and both orders of the z sum spread 5.3e-15 on the CPU): dense storage
   (gemv_variant -1, 0, 20421) and CSR, one shard and 2 / 3 loopback shards (1000 / 3 cuts blocks at shard boundaries), and one
   case through the RCCL transport's test double.
3. Iteration counts at tol = 1e-6 ||b|| on lap2d n = 1024: 67 / 55 / 39 / 29 for block 4 / 64 / 128 / 256 (plain and point Jacobi:
   90), reproduced by the fp64 and the longdouble reference with the residual at most 0.91 tol at the stop and at least 1.08 tol
   one step before: no rounding tie.
4. What it is for: 4 unknowns per node with ill-scaled node blocks -- 54 iterations at block 4, 41 at block 16, point Jacobi more
   than 4 times as many as block 4.
5. Exact after one iteration on a block-diagonal matrix.
6. Bit identity under row-varying powers of two: block Jacobi on (S L S, S b) is S^-1 x of block Jacobi on (L, b) bit for bit
   (the argument of tests/test_gpu_jacobi_scaled.py; the inversion has no pivoting, the z chain a fixed order).  A W read at the
   wrong row, a wrong block start or a stale W breaks it.
7. Staleness and the default.  8. Errors and refusals, and the fault walk over a begin."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import block_jacobi_reference as ref
import test_gpu_csr as tc
from test_gpu_jacobi import fake_rccl_dir  # noqa: F401  (the module-scoped fixture that builds tests/fake_rccl)
from test_gpu_jacobi_scaled import _write_mtx

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "conjugate-gradient_amd", "cgsolver")
SEED = 0x3D1F
BAD_ARG, ERR_HIP, UNSUPPORTED = 1, 3, 7
REL_BOUND = 1e-10
EPS = 2.0 ** -52
LD = np.longdouble


def _oracle():
    import __graft_entry__ as g
    O = g.load_oracle()
    O.build()
    return O


def _diag(n):
    return 1.03 * 2.0 * np.sqrt(n / 3.0)   # tests/test_gpu_multi_rhs.py: the symmetric hash matrix is SPD


@functools.lru_cache(maxsize=None)
def _matrix(name):
    """(A, b) of a named test problem, read-only."""
    O = _oracle()
    if name.startswith("lap2d"):
        n = int(name[5:])
        A, b = O.generate_lap2d(n), O.init_source_term(n)
    elif name.startswith("hash"):
        n = int(name[4:])
        A, b = O.hash_rows(n, 0, n, SEED, True, _diag(n)), O.init_source_term(n)
    else:
        assert name == "dof4"
        A, b = ref.four_dof_matrix(O.generate_lap2d(256))
    assert np.array_equal(A, A.T)
    A.setflags(write=False)
    b.setflags(write=False)
    return A, b


@functools.lru_cache(maxsize=None)
def _reference(name, block, iters, tol, keep=()):
    A, b = _matrix(name)
    return ref.pcg(A, b, block, iters, tol, LD, keep)


def _solver(pkg, storage, p=1, variant=0, **kw):
    mode = pkg.COMM_SELF if p == 1 else pkg.COMM_LOOPBACK
    fmt = pkg.MATRIX_CSR if storage == "csr" else pkg.MATRIX_DENSE
    return pkg.CGSolver(comm_mode=mode, nranks=p, matrix_format=fmt, gemv_variant=variant, **kw)


def _load(c, storage, A):
    if storage == "csr":
        c.set_matrix_csr(*tc.dense_to_csr(A))
    else:
        c.set_matrix_dense(A)


def _solve(c, b, iters, tol=0.0):
    c.set_max_iter(iters)
    c.tolerance(tol)
    c.set_source_term(b)
    x = np.zeros(len(b))
    return x, c.solve(x)


def _begin(c, b):
    """A begin alone (it makes the block inverses), ended at once."""
    c.set_max_iter(1)
    c.set_source_term(b)
    c.solve_begin(np.zeros(len(b)))
    c.solve_end(np.zeros(len(b)))


# ---- 1. the inverse alone ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", ["dense", "csr"])
@pytest.mark.parametrize("name,block", [("lap2d257", 256)] + [("lap2d1000", b) for b in (2, 8, 64, 256)]
                         + [("hash600", b) for b in (8, 128, 256)])
def test_inverse_alone(gpu_pkg, name, block, storage):
    A, b = _matrix(name)
    with _solver(gpu_pkg, storage) as c:
        _load(c, storage, A)
        c.set_preconditioner("jacobi", block=block)
        assert c.preconditioner_block() == block
        _begin(c, b)
        W = c._probe_precond_blocks()
    _check_inverse(W, A, block, (name, storage))


def _check_inverse(W, A, block, what):
    """The block inverses as cgx_probe_get_precond_blocks returns them, against the diagonal blocks of A (item 1 of the header)."""
    n = A.shape[0]
    assert W.shape == (n, block)
    worst = 0.0
    for s, e in ref.block_ranges(n, block):
        m = e - s
        Wb = W[s:e, :m]
        assert np.array_equal(Wb.view(np.uint64), Wb.T.copy().view(np.uint64)), (s, "not symmetric bit for bit")
        assert not W[s:e, m:].any(), (s, "not zero outside the block")
        D = A[s:e, s:e]
        err = float(np.max(np.abs(Wb.astype(LD) @ D.astype(LD) - np.eye(m, dtype=LD))))
        bar = 4 * m * EPS * float(np.linalg.cond(D, 2))
        worst = max(worst, err / bar)
        assert err <= bar, (s, m, err, bar)
    print("inverse %r block %d: worst max|W D - I| / (4 m eps kappa) = %.3f" % (what, block, worst))


# ---- 2. fixed iterations against the longdouble PCG --------------------------------------------------------------------------
FIXED = [("lap2d1000", b) for b in (4, 32, 256)] + [("hash600", b) for b in (8, 64, 128)] + [("dof4", b) for b in (4, 16)]
PATHS = [("dense", -1), ("dense", 0), ("dense", 20421), ("csr", 0)]


@pytest.mark.parametrize("p", [1, 2, 3])
@pytest.mark.parametrize("name,block", FIXED)
def test_fixed_iterations_against_longdouble(gpu_pkg, name, block, p):
    A, b = _matrix(name)
    want = _reference(name, block, 40, 0.0, (12, 40))["xs"]
    for storage, variant in PATHS:
        with _solver(gpu_pkg, storage, p, variant) as c:
            _load(c, storage, A)
            c.set_preconditioner("jacobi", block=block)
            for k in (12, 40):
                x, res = _solve(c, b, k)
                err = float(np.linalg.norm(x - want[k]) / np.linalg.norm(want[k]))
                print("fixed %s block %d %s/%d p=%d k=%d: |x - x_ref| / |x_ref| = %.3e" % (name, block, storage, variant, p, k, err))
                assert res["iterations"] == k, res
                assert err <= REL_BOUND, (storage, variant, k, err)


def _longdouble_line(A, b, block, iters):
    """||x|| and sqrt(r.r) after the last update, as the CLI prints them after a loop that ran out."""
    o = ref.pcg(A, b, block, iters, 0.0, LD)
    return float(np.linalg.norm(o["x"].astype(LD))), o["residual_last"]


def test_rccl_transport_against_longdouble(gpu_pkg, fake_rccl_dir, tmp_path):  # noqa: F811
    """`cgsolver FILE OUT 40 --gpus 2 --transport rccl --jacobi-block 32` on lap2d n = 1000 from a file (far from converged after
    40 iterations): the printed ||x|| and residual against the longdouble PCG, 2e-6 relative -- what seven printed digits allow
    (the bar of tests/test_gpu_rccl_path.py)."""
    A, b = _matrix("lap2d1000")
    iters, block = 40, 32
    path = _write_mtx(tmp_path / "lap2d.mtx", A)
    xn_ref, res_ref = _longdouble_line(A, b, block, iters)
    env = dict(os.environ, LD_LIBRARY_PATH=fake_rccl_dir + os.pathsep + os.environ.get("LD_LIBRARY_PATH", ""))
    r = subprocess.run([EXE, path, str(tmp_path / "out"), str(iters), "--gpus", "2", "--same-device", "--transport", "rccl",
                        "--jacobi-block", str(block), "--stats"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "fake_rccl: rank 1 of 2 wired" in r.stderr, r.stderr[-2000:]
    stats = re.search(r"cgsolver stats: .*", r.stderr).group(0)
    assert stats.endswith("precond=jacobi block=32") and " gpus=2 " in stats, stats
    mm = re.search(r"\[STEP (\d+)\] residual = (\S+), \|\|x\|\| = (\S+),", r.stdout)
    assert mm, r.stdout
    k, res, xn = int(mm.group(1)), float(mm.group(2)), float(mm.group(3))
    print("cli rccl: k=%d residual %.6e (reference %.9e) ||x|| %.6e (reference %.9e)" % (k, res, res_ref, xn, xn_ref))
    assert k == iters
    assert abs(xn - xn_ref) <= 2e-6 * xn_ref, (xn, xn_ref)
    assert abs(res - res_ref) <= 2e-6 * res_ref, (res, res_ref)


# ---- 3. iteration counts -----------------------------------------------------------------------------------------------------
def _count_reference(name, block, want):
    """The fp64 and the longdouble reference both stop at `want`, away from a rounding tie; returns the longdouble one."""
    A, b = _matrix(name)
    n = len(b)
    tol = 1e-6 * float(np.linalg.norm(b))
    o64 = ref.pcg(A, b, block, n, tol, np.float64)
    old = _reference(name, block, n, tol)
    for o in (o64, old):
        assert o["converged"] == 1 and o["iterations"] == want, (block, o["iterations"], want)
        assert o["residual_last"] <= 0.91 * tol and o["residual_prev"] >= 1.08 * tol, (o["residual_last"] / tol, o["residual_prev"] / tol)
    return tol, old


def _check_count(res, tol, old, want):
    assert res["converged"] == 1 and res["iterations"] == want, res
    assert res["residual_last"] < tol <= res["residual_prev"], (res, tol)
    assert abs(res["residual_prev"] - old["residual_prev"]) <= 1e-9 * old["residual_prev"], (res, old["residual_prev"])


@pytest.mark.parametrize("block,want", [(4, 67), (64, 55), (128, 39), (256, 29)])
def test_iteration_counts_on_lap2d(gpu_pkg, block, want):
    tol, old = _count_reference("lap2d1024", block, want)
    A, b = _matrix("lap2d1024")
    with _solver(gpu_pkg, "dense") as c:
        c.generate_lap2d_matrix(1024)
        c.set_preconditioner("jacobi", block=block)
        c.set_max_iter(1024)
        c.tolerance(tol)
        c.init_source_term(1.0 / 1024)
        res = c.solve(np.zeros(1024))
    _check_count(res, tol, old, want)


# ---- 4. it does its job ------------------------------------------------------------------------------------------------------
def test_four_unknowns_per_node(gpu_pkg):
    A, b = _matrix("dof4")
    n = len(b)
    got = {}
    for block, want in ((4, 54), (16, 41)):
        tol, old = _count_reference("dof4", block, want)
        with _solver(gpu_pkg, "dense") as c:
            c.set_matrix_dense(A)
            c.set_preconditioner("jacobi", block=block)
            _, res = _solve(c, b, n, tol)
        _check_count(res, tol, old, want)
        got[block] = res["iterations"]
    with _solver(gpu_pkg, "dense") as c:
        c.set_matrix_dense(A)
        c.set_preconditioner("jacobi")
        _, point = _solve(c, b, 4 * n, tol)
    print("4 unknowns per node: point Jacobi %d iterations, block 4 %d, block 16 %d" % (point["iterations"], got[4], got[16]))
    assert point["converged"] == 0 or point["iterations"] > 4 * got[4], (point, got)


# ---- 5. exact on a block-diagonal matrix -------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", ["dense", "csr"])
@pytest.mark.parametrize("block,n", [(8, 300), (64, 300), (256, 600)])
def test_exact_on_a_block_diagonal_matrix(gpu_pkg, block, n, storage):
    A, b = ref.block_diagonal_matrix(n, block, 1000 * block + n)
    with _solver(gpu_pkg, storage) as c:
        _load(c, storage, A)
        c.set_preconditioner("jacobi", block=block)
        x, res = _solve(c, b, 1)
        c.set_preconditioner("jacobi")
        _, point = _solve(c, b, 1)
    print("block diagonal %d/%d %s: rel_residual %.3e after one iteration (point Jacobi %.3e)" % (
        block, n, storage, res["rel_residual"], point["rel_residual"]))
    assert res["iterations"] == 1 and res["rel_residual"] <= 1e-12, res
    assert point["rel_residual"] > 1e-3, point


# ---- 6. bitwise, row-varying powers of two ------------------------------------------------------------------------------------
def _scale(n, seed):
    rng = np.random.default_rng(seed)
    e = rng.permutation(np.arange(n) % 7 - 3)   # every exponent of [-3, 3], permuted
    assert e.min() == -3 and e.max() == 3
    return np.ldexp(1.0, e)


SCALED_PATHS = [("dense", -1, 1), ("dense", 0, 1), ("dense", 20421, 1), ("csr", 0, 1), ("dense", 0, 3), ("csr", 0, 3)]


@pytest.mark.parametrize("block", [2, 8, 64, 256])
def test_scaled_rows_give_the_unscaled_bits(gpu_pkg, block):
    n, iters = 1000, 30
    L, bt = _matrix("lap2d1000")
    s = _scale(n, block)
    A = (s[:, None] * L) * s[None, :]
    assert np.array_equal(A, A.T)
    for storage, variant, p in SCALED_PATHS:
        xs = []
        for M, b in ((L, bt), (A, s * bt)):
            with _solver(gpu_pkg, storage, p, variant) as c:
                _load(c, storage, M)
                c.set_preconditioner("jacobi", block=block)
                x, res = _solve(c, b, iters)
                assert res["iterations"] == iters and res["converged"] == 0, res
                xs.append(x)
        xt, xj = xs
        assert np.all(np.isfinite(xt)) and np.all(np.isfinite(xj)) and np.linalg.norm(xt) > 0
        sx = s * xj
        same = np.array_equal(sx.view(np.uint64), xt.view(np.uint64))
        print("scaled block %d %s/%d p=%d: same=%s |s x_S - x| / |x| = %.3e" % (
            block, storage, variant, p, same, np.linalg.norm(sx - xt) / np.linalg.norm(xt)))
        assert same, (storage, variant, p, int(np.count_nonzero(sx != xt)))


# ---- 7. staleness and the default --------------------------------------------------------------------------------------------
def _bits(a, b):
    (xa, ra), (xb, rb) = a, b
    assert np.array_equal(xa.view(np.uint64), xb.view(np.uint64)), np.max(np.abs(xa - xb))
    for key in ("iterations", "converged", "residual_prev", "residual_last", "rel_residual", "x_norm"):
        assert ra[key] == rb[key], (key, ra[key], rb[key])


def _fresh(pkg, A, b, block, iters=30, p=1):
    with _solver(pkg, "dense", p) as c:
        c.set_matrix_dense(A)
        c.set_preconditioner("jacobi", block=block)
        return _solve(c, b, iters)


def test_default_and_block_one_are_todays_jacobi(gpu_pkg):
    A, b = _matrix("hash600")
    L = gpu_pkg.cgx.lib()
    with _solver(gpu_pkg, "dense") as c:
        c.set_matrix_dense(A)
        assert c.preconditioner_block() == 1
        assert L.cgx_set_preconditioner(c._h, 1) == 0     # the kind alone, the setter of the block never called
        today = _solve(c, b, 30)
        with pytest.raises(gpu_pkg.CgxError) as e:        # no block inverses at block 1
            c._probe_precond_blocks()
        assert e.value.status == BAD_ARG
    _bits(_fresh(gpu_pkg, A, b, 1), today)
    with _solver(gpu_pkg, "dense") as c:                  # block 1 after a block > 1 on the same matrix
        c.set_matrix_dense(A)
        c.set_preconditioner("jacobi", block=8)
        other = _solve(c, b, 30)
        c.set_preconditioner("jacobi", block=1)
        _bits(_solve(c, b, 30), today)
    assert not np.array_equal(other[0], today[0])


@pytest.mark.parametrize("p", [1, 3])
def test_a_second_matrix_and_a_new_block_size_leave_nothing_behind(gpu_pkg, p):
    A1, b = _matrix("hash600")
    s = _scale(600, 5)
    A2 = (s[:, None] * A1) * s[None, :]
    with _solver(gpu_pkg, "dense", p) as c:
        c.set_matrix_dense(A1)
        c.set_preconditioner("jacobi", block=64)
        first = _solve(c, b, 30)
        c.set_matrix_dense(A2)                            # a second matrix: the setting survives, W is made again
        assert c.preconditioner_block() == 64
        second = _solve(c, b, 30)
        c.set_preconditioner("jacobi", block=8)           # a new block size on the same matrix
        third = _solve(c, b, 30)
        c.set_preconditioner("jacobi", block=64)
        fourth = _solve(c, b, 30)
    _bits(first, _fresh(gpu_pkg, A1, b, 64, p=p))
    _bits(second, _fresh(gpu_pkg, A2, b, 64, p=p))
    _bits(third, _fresh(gpu_pkg, A2, b, 8, p=p))
    _bits(fourth, second)
    assert not np.array_equal(first[0], second[0]) and not np.array_equal(second[0], third[0])


# ---- 8. errors ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [1, 3])
def test_an_indefinite_block_is_refused_and_the_context_stays_usable(gpu_pkg, p):
    n = 64
    O = _oracle()
    A = O.generate_lap2d(n)
    A[10:12, 10:12] = [[1.0, 2.0], [2.0, 1.0]]            # the diagonal is positive: point Jacobi accepts it
    b = O.init_source_term(n)
    # This A is indefinite (smallest eigenvalue -1.55), so CG on it is only defined while p.Ap > 0.  With point Jacobi p.Ap is
    # 1.4e6, 4.2e6, 6.3e6 in iterations 0 - 2 and -1.3e7 in iteration 3 (fp64 and longdouble agree to 15 digits); there the
    # library's alpha = rsold / max(p.Ap, rsold * 1e-10) (cg.cc:107) is 1e10 and every path overflows to NaN a few steps later.
    # So the solve that follows the refusal runs the 3 iterations that are defined.
    iters = 3
    want = ref.pcg(A, b, 1, iters, 0.0, LD)
    with _solver(gpu_pkg, "dense", p) as c:
        c.set_matrix_dense(A)
        c.set_preconditioner("jacobi", block=2)
        for _ in range(2):                                # still refused: the check runs again
            with pytest.raises(gpu_pkg.CgxError) as e:
                _solve(c, b, iters)
            assert e.value.status == BAD_ARG and "row 10" in str(e.value), str(e.value)
        c.set_preconditioner("jacobi", block=1)
        x, res = _solve(c, b, iters)
        assert res["iterations"] == iters
    assert np.all(np.isfinite(x)) and np.isfinite(res["residual_last"]), res
    assert np.linalg.norm(x - want["x"]) <= REL_BOUND * np.linalg.norm(want["x"])
    _bits((x, res), _fresh(gpu_pkg, A, b, 1, iters, p))


def test_setter_is_refused_inside_a_solve(gpu_pkg):
    n = 1024
    L = gpu_pkg.cgx.lib()
    with _solver(gpu_pkg, "dense", variant=-1) as c:
        c.generate_lap2d_matrix(n)
        c.init_source_term(1.0 / n)
        c.set_preconditioner("jacobi", block=4)
        assert L.cgx_set_preconditioner_block(c._h, 3) == BAD_ARG
        c.solve_begin(np.zeros(n))
        assert L.cgx_set_preconditioner_block(c._h, 8) == BAD_ARG
        c.solve_steps(5)
        c.solve_end(np.zeros(n))
        assert c.preconditioner_block() == 4
        assert L.cgx_set_preconditioner_block(c._h, 8) == 0


def test_unsupported_combinations(gpu_pkg, monkeypatch):
    monkeypatch.delenv("CGX_RESIDENT", raising=False)
    n = 2048
    with gpu_pkg.CGSolver() as c:
        c.generate_lap2d_matrix(n)
        c.init_source_term(1.0 / n)
        c.set_preconditioner("jacobi", block=16)
        with pytest.raises(gpu_pkg.CgxError) as e:
            c.solve_multi(np.ones((2, n)))
        assert e.value.status == UNSUPPORTED
    with gpu_pkg.CGSolver(matrix_format=gpu_pkg.MATRIX_BANDED) as c:
        c.generate_lap2d_matrix(n)
        c.init_source_term(1.0 / n)
        c.set_preconditioner("jacobi", block=16)
        with pytest.raises(gpu_pkg.CgxError) as e:
            c.solve(np.zeros(n))
        assert e.value.status == UNSUPPORTED
    with gpu_pkg.CGSolver(gemv_variant=40000) as c:
        c.generate_lap2d_matrix(n)
        c.init_source_term(1.0 / n)
        c.set_preconditioner("jacobi", block=16)
        with pytest.raises(gpu_pkg.CgxError) as e:
            c.solve(np.zeros(n))
        assert e.value.status == UNSUPPORTED


def test_fused_p2p_update_refuses_a_block(gpu_pkg):
    """A one-rank CGX_COMM_P2P context: the exchange folded into the update kernel has no block form (every rank passes the same
    block, so every rank refuses); with the exchange in its own kernel the ordinary update kernel runs and the block is taken."""
    n = 1024
    A, b = _matrix("lap2d1024")
    with gpu_pkg.CGSolver(comm_mode=gpu_pkg.COMM_P2P, nranks=1) as c:
        c.generate_lap2d_matrix(n)
        c.init_source_term(1.0 / n)
        c.set_max_iter(20)
        c.set_preconditioner("jacobi", block=32)
        with pytest.raises(gpu_pkg.CgxError) as e:
            c.solve(np.zeros(n))
        assert e.value.status == UNSUPPORTED
        c.set_preconditioner("jacobi", block=1)           # the context stays usable
        assert c.solve(np.zeros(n))["iterations"] == 20
    with gpu_pkg.CGSolver(comm_mode=gpu_pkg.COMM_P2P, nranks=1, p2p_separate_exchange=True) as c:
        c.generate_lap2d_matrix(n)
        c.set_preconditioner("jacobi", block=32)
        x, res = _solve(c, b, 20)
    want = ref.pcg(A, b, 32, 20, 0.0, LD)["x"]
    assert np.linalg.norm(x - want) <= REL_BOUND * np.linalg.norm(want)


def test_fault_walk_over_a_begin(gpu_pkg):
    import torch
    A, b = _matrix("hash600")
    n = len(b)
    with _solver(gpu_pkg, "dense") as c:
        c.set_matrix_dense(A)
        c.set_preconditioner("jacobi", block=64)
        ref_run = _solve(c, b, 20)
        c.set_preconditioner("jacobi", block=32)          # W goes stale (nothing is allocated before the next begin) ...
        c.set_preconditioner("jacobi", block=64)          # ... so the begins below extract and invert again
        free0 = torch.cuda.mem_get_info()[0]
        calls = 0
        while True:
            c._set_fault_after(calls)
            try:
                c.solve_begin(np.zeros(n))
            except gpu_pkg.CgxError as e:
                assert e.status == ERR_HIP, (calls, e)
                assert torch.cuda.mem_get_info()[0] == free0, calls
                calls += 1
                assert calls < 300
                continue
            c._set_fault_after(-1)
            break
        assert calls > 8, calls
        c.solve_steps(20)
        x = np.zeros(n)
        res = c.solve_end(x)
        _bits((x, res), ref_run)
        _bits(_solve(c, b, 20), ref_run)
