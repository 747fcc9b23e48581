"""Jacobi PCG with a diagonal that differs in every row, on every path that applies dinv (DESIGN.md sections 11 and 12).

tests/test_gpu_jacobi.py and tests/test_gpu_csr.py show "Jacobi on a matrix whose diagonal is one power of two gives the plain
bits".  On such a matrix every dinv[i] is the same number, so a dinv read at the wrong row, gathered from the shards in the wrong
order or left over from the previous matrix is invisible.  Here:

1. Bit identity with a non-uniform diagonal.  L has one power of two c on its diagonal (generate_lap2d: 4; the symmetric hash
   matrix with diag = 2**k), s_i = 2**e_i with integer e_i in [-8, 8] that differ from row to row, A = S L S, b = S b~.  Then
   r = S r~, z = r~ / (c s), p = S^-1 p~ / c, alpha_J = c alpha, rho = r~.r~ / c and x = S^-1 x~ hold in floating point: every
   relation is a scaling by a power of two, which commutes with every rounding and every fma, whatever the summation order of a
   row of A p (tests/test_oracle.py test_power_of_two_scaling_commutes_with_jacobi_pcg pins this on the CPU).  So s * x_jacobi
   must equal x_plain BIT FOR BIT when both runs use the same storage, K1 shape and transport, tol = 0 (the stopping test sees
   r.r, which is not scaled uniformly) and the same number of iterations -- through the per-launch K1 shapes, variant 6,
   loopback shards, CSR up to n = 2**20 (k_update_xr_strided_pc, the long loop of head_finish_pc, the grid-stride trips of
   k_init_residual_pc / k_jacobi_dinv / k_csr_diag_slice), P2P processes, and a second matrix on the same context.
2. Diagonals that are not powers of two against tests/test_gpu_jacobi.py's longdouble PCG, on loopback shards, the one-round and
   column-split K1 shapes and through the CLI on the RCCL (test double) and loopback transports.

Every Jacobi run's rel_residual is compared with ||A x - b|| / ||b|| recomputed on the host from the returned x: 1e-9 relative
(the bar of tests/test_gpu_parity.py test_full_size_properties) plus what two fp64 evaluations of A x - b may themselves be off
by, (m + 2) eps (|A||x| + |b|) per row of m entries -- the hash-matrix runs converge long before their last iteration, and there
the quantity is that rounding error and nothing else.
Every test asserts the plan or path it means to run."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import test_gpu_csr as tc
import test_gpu_jacobi as tj
from test_gpu_jacobi import fake_rccl_dir  # noqa: F401  (the module-scoped fixture that builds tests/fake_rccl)

pytestmark = pytest.mark.gpu

ROOT = tj.ROOT
EXE = tj.EXE
SEED = tj.SEED
EPS = float(np.finfo(np.float64).eps)
N_STRIDED = 262144   # 256 * kMaxVectorGrid (cgx_kernels.h): above it K3 strides and the head folds more than 256 partials


# ---- helpers -----------------------------------------------------------------------------------------------------------------
def _scale(n, seed):
    """s_i = 2**e_i, e_i uniform in [-8, 8], not all equal."""
    e = np.random.default_rng(seed).integers(-8, 9, n)
    assert len(set(e.tolist())) > 1 and e.min() >= -8 and e.max() <= 8
    return np.ldexp(1.0, e)


def _sls_dense(L, s):
    return (s[:, None] * L) * s[None, :]


def _hash_diag(n):
    return float(2 ** int(np.ceil(np.log2(n + 1))))


def _assert_same_bits(s, xj, xt, what=None):
    """s * x_jacobi == x_plain on all n entries; NaNs would compare equal as bit patterns, so finiteness is asserted first."""
    assert np.all(np.isfinite(xt)) and np.all(np.isfinite(xj)) and np.linalg.norm(xt) > 0, what
    sx = s * xj
    same = np.array_equal(sx.view(np.uint64), xt.view(np.uint64))
    diff = np.linalg.norm(sx - xt) / np.linalg.norm(xt)
    print("bits %r: same=%s |s x_J - x~| / |x~| = %.3e" % (what, same, diff))
    assert same, (what, diff, int(np.count_nonzero(sx != xt)))


def _dense_products(A, x, chunk=2048):
    """A x and |A| |x| in fp64, row block by row block (no second copy of a 2 GB matrix)."""
    ax, absx = np.empty(len(x)), np.abs(x)
    aax = np.empty(len(x))
    for i in range(0, len(x), chunk):
        blk = A[i:i + chunk]
        ax[i:i + chunk] = blk @ x
        aax[i:i + chunk] = np.abs(blk) @ absx
    return ax, aax


def _row_entries(A, chunk=2048):
    """The most non-zeros in a row: a product with an exact zero adds nothing to a row sum in any order."""
    return max(int(np.count_nonzero(A[i:i + chunk], axis=1).max()) for i in range(0, A.shape[0], chunk))


def _csr_products(rows, indices, data, x, n):
    return (np.bincount(rows, weights=data * x[indices], minlength=n),
            np.bincount(rows, weights=np.abs(data) * np.abs(x[indices]), minlength=n))


def _check_rel_residual(res, ax, aax, b, row_entries, what=None):
    nb = np.linalg.norm(b)
    ref = float(np.linalg.norm(ax - b) / nb)
    floor = float(np.linalg.norm((row_entries + 2) * EPS * (aax + np.abs(b))) / nb)
    print("rel_residual %r: reported %.17g host %.17g rounding allowance %.3e" % (what, res["rel_residual"], ref, 2 * floor))
    assert abs(res["rel_residual"] - ref) <= 1e-9 * ref + 2 * floor, (what, res["rel_residual"], ref, floor)


def _solve(c, b, iters, jacobi, tol=0.0):
    c.set_preconditioner("jacobi" if jacobi else None)
    assert c.preconditioner == ("jacobi" if jacobi else None)
    c.set_max_iter(iters)
    c.tolerance(tol)
    c.set_source_term(b)
    x = np.zeros(len(b))
    res = c.solve(x)
    if tol == 0.0:
        assert res["iterations"] == iters and res["converged"] == 0, res
    return x, res


def _shards(c):
    """The number of local shards: gemv_plan answers for exactly those."""
    p = 0
    while True:
        try:
            c.gemv_plan(p)
        except Exception:   # noqa: BLE001 -- CgxError of the package under test
            return p
        p += 1
        assert p <= 64


def _dense_pair(pkg, L, s, bt, iters, check_plan, what, **kw):
    """Plain CG on (L, b~) and Jacobi on (S L S, S b~), each on a fresh context made alike; L is uploaded as S L S is."""
    with pkg.CGSolver(**kw) as c:
        c.set_matrix_dense(L)
        check_plan(c)
        xt, _ = _solve(c, bt, iters, False)
    A = _sls_dense(L, s)
    assert np.array_equal(A, A.T)
    with pkg.CGSolver(**kw) as c:
        c.set_matrix_dense(A)
        c.set_preconditioner("jacobi")
        check_plan(c)
        xj, rj = _solve(c, s * bt, iters, True)
        check_plan(c)
    _assert_same_bits(s, xj, xt, what)
    ax, aax = _dense_products(A, xj)
    _check_rel_residual(rj, ax, aax, s * bt, _row_entries(A), what)
    return xt, xj, rj


# ---- 1a. dense, one GPU, the per-launch K1 shapes ---------------------------------------------------------------------------
# gemv_variant = variant * 10000 + R * 100 + U * 10 + d (plan_gemv, cgx_kernels.hip): d = 2 the one-round form, 3 / 4 / 5 the same
# with the columns of a row group split 2 / 4 / 8 ways.  What cgx_get_gemv_plan must report for each: (variant, R, U, light, split)
DENSE_SHAPES = {10821: (1, 8, 2, 0, 1), 20421: (2, 4, 2, 0, 1), 10822: (1, 8, 2, 1, 1), 10442: (1, 4, 4, 1, 1),
                10823: (1, 8, 2, 1, 2), 10444: (1, 4, 4, 1, 4), 10445: (1, 4, 4, 1, 8)}


def _shape_check(code):
    def check(c):
        plan = c.gemv_plan()
        assert tuple(plan[k] for k in ("variant", "R", "U", "light", "split")) == DENSE_SHAPES[code], (code, plan)
        assert _shards(c) == 1
    return check


@functools.lru_cache(maxsize=2)
def _small_l(matrix, n):
    import __graft_entry__ as g
    O = g.load_oracle()
    L = O.generate_lap2d(n) if matrix == "lap2d" else O.hash_rows(n, 0, n, SEED, True, _hash_diag(n))
    c = L[0, 0]
    assert np.all(np.diag(L) == c) and c == 2.0 ** int(np.log2(c)) and np.array_equal(L, L.T)
    L.setflags(write=False)
    return L


@pytest.mark.parametrize("variant", sorted(DENSE_SHAPES))
@pytest.mark.parametrize("matrix", ["lap2d", "hash"])
def test_dense_shapes_scaled_diagonal_gives_the_plain_bits(gpu_pkg, oracle, matrix, variant):
    n, iters = 4096, 40
    _dense_pair(gpu_pkg, _small_l(matrix, n), _scale(n, n + variant), oracle.init_source_term(n), iters, _shape_check(variant),
                (matrix, variant), gemv_variant=variant)


# ---- 1b. variant 6 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("matrix,n", [("lap2d", 16900), ("hash", 16385)])
def test_variant6_scaled_diagonal_gives_the_plain_bits(gpu_pkg, oracle, matrix, n):
    """k_pcg_symv_tiles + fold: the symmetry check must accept S L S (exactly symmetric), and the transposed column pieces of a
    far tile scale with their own row.  One host copy of the matrix at a time: L is scaled in place after the plain run."""
    iters = 40
    _small_l.cache_clear()
    if matrix == "lap2d":
        L = oracle.generate_lap2d(n)
    else:
        oracle.set_threads(16)
        try:
            L = oracle.hash_rows(n, 0, n, SEED, True, _hash_diag(n))
        finally:
            oracle.set_threads(1)
    assert np.all(np.diag(L) == L[0, 0]) and L[0, 0] in (4.0, 32768.0)
    s = _scale(n, n)
    bt = oracle.init_source_term(n)
    with gpu_pkg.CGSolver(gemv_variant=-1) as c:
        c.set_matrix_dense(L)
        assert c.gemv_plan()["variant"] == 6, c.gemv_plan()
        xt, _ = _solve(c, bt, iters, False)
    L *= s[:, None]
    L *= s[None, :]
    A = L
    with gpu_pkg.CGSolver(gemv_variant=-1) as c:
        c.set_matrix_dense(A)
        c.set_preconditioner("jacobi")
        assert c.gemv_plan()["variant"] == 6, c.gemv_plan()
        xj, rj = _solve(c, s * bt, iters, True)
        assert c.gemv_plan()["variant"] == 6
    _assert_same_bits(s, xj, xt, (matrix, n))
    ax, aax = _dense_products(A, xj)
    _check_rel_residual(rj, ax, aax, s * bt, _row_entries(A), (matrix, n))


# ---- 1c. loopback shards, dense ----------------------------------------------------------------------------------------------
def _loopback_check(pkg, p):
    def check(c):
        info = c.comm_info()
        assert _shards(c) == p and info["comm_mode"] == pkg.COMM_LOOPBACK and info["ranks_wired"] == p, info
        assert all(c.gemv_plan(q)["variant"] == 1 for q in range(p))
    return check


@pytest.mark.parametrize("n,p", [(4096, 2), (3001, 3), (2048, 8), (5, 8)])   # (5, 8): every shard but the last is empty
def test_loopback_shards_scaled_diagonal_gives_the_plain_bits(gpu_pkg, oracle, n, p):
    """k_update_xr_pc with row0 > 0 and the diagonal gathered through gather_segments."""
    iters = 3 if n < 16 else 60
    _dense_pair(gpu_pkg, oracle.generate_lap2d(n), _scale(n, 31 * n + p), oracle.init_source_term(n), iters,
                _loopback_check(gpu_pkg, p), (n, p), comm_mode=gpu_pkg.COMM_LOOPBACK, nranks=p)


# ---- 1d. CSR -----------------------------------------------------------------------------------------------------------------
def _csr_rows(indptr):
    return np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))


def _csr_check(p, L=0):
    def check(c):
        assert _shards(c) == p
        for q in range(p):
            plan = c.gemv_plan(q)
            assert plan["variant"] == 7 and (L == 0 or plan["R"] == L - 70000), plan
    return check


def _csr_run(pkg, p, L, csr, b, iters, jacobi, **kw):
    with tc.solver(pkg, p, gemv_variant=L, **kw) as c:
        c.set_matrix_csr(*csr)
        _csr_check(p, L)(c)
        assert c.matrix_nnz(0) > 0 and sum(c.matrix_nnz(q) for q in range(p)) == len(csr[2])
        return _solve(c, b, iters, jacobi)


@pytest.mark.parametrize("p,L", [(1, 0), (3, 0), (1, 70016), (3, 70002)])
def test_csr_scaled_diagonal_gives_the_plain_bits(gpu_pkg, oracle, p, L):
    n, iters = 4096, 120
    indptr, indices, data = tc.lap2d_csr(n)
    rows = _csr_rows(indptr)
    s = _scale(n, 7 * n + p + L)
    bt = oracle.init_source_term(n)
    scaled = s[rows] * data * s[indices]
    xt, _ = _csr_run(gpu_pkg, p, L, (indptr, indices, data), bt, iters, False)
    xj, rj = _csr_run(gpu_pkg, p, L, (indptr, indices, scaled), s * bt, iters, True)
    _assert_same_bits(s, xj, xt, (p, L))
    ax, aax = _csr_products(rows, indices, scaled, xj, n)
    _check_rel_residual(rj, ax, aax, s * bt, 5, (p, L))


N20 = 1 << 20


@pytest.fixture(scope="module")
def perm20(oracle):
    """The permuted lap2d of tests/test_gpu_csr.py test_permuted_lap2d_at_2_pow_20 (which ties its plain run to
    oracle.solve_lap2d_banded) and its permuted source term."""
    perm = np.random.default_rng(20261016).permutation(N20)
    indptr, indices, data = tc.lap2d_csr(N20, perm)
    bp = np.empty(N20)
    bp[perm] = oracle.init_source_term(N20)
    return indptr, indices, data, _csr_rows(indptr), bp


_PLAIN20 = {}


def _plain20(pkg, perm20, p):
    if p not in _PLAIN20:
        indptr, indices, data, _, bp = perm20
        _PLAIN20[p] = _csr_run(pkg, p, 0, (indptr, indices, data), bp, 200, False)[0]
    return _PLAIN20[p]


@pytest.mark.parametrize("p", [1, 3])
@pytest.mark.parametrize("diagonal", ["scaled", "uniform"])
def test_csr_2_pow_20_gives_the_plain_bits(gpu_pkg, perm20, p, diagonal):
    """n = 2**20 > 256 * kMaxVectorGrid: K3 is k_update_xr_strided_pc, head_finish_pc folds 1024 partials per set in its second
    loop, and k_init_residual_pc, k_jacobi_dinv and k_csr_diag_slice take grid-stride trips.  "uniform": Jacobi on the
    unscaled matrix (diagonal 4) gives the plain bits; "scaled": data = s[row] v s[col]."""
    n, iters = N20, 200
    assert n > N_STRIDED and n == 2 ** 20
    indptr, indices, data, rows, bp = perm20
    assert len(indptr) == n + 1
    s = _scale(n, n + p) if diagonal == "scaled" else np.ones(n)
    scaled = s[rows] * data * s[indices]
    xt = _plain20(gpu_pkg, perm20, p)
    xj, rj = _csr_run(gpu_pkg, p, 0, (indptr, indices, scaled), s * bp, iters, True)
    _assert_same_bits(s, xj, xt, (p, diagonal))
    ax, aax = _csr_products(rows, indices, scaled, xj, n)
    _check_rel_residual(rj, ax, aax, s * bp, 5, (p, diagonal))


# ---- 1e. P2P processes -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("worker,tagged,port", [("p2p_jacobi_worker.py", 0, 29783), ("p2p_jacobi_worker.py", 1, 29784),
                                                ("p2p_csr_worker.py", 0, 29793), ("p2p_csr_worker.py", 1, 29794)])
def test_p2p_processes_scaled_diagonal_gives_the_plain_bits(tmp_path, worker, tagged, port):
    """k_pcg_update_p2p in the flag form and the tagged form, the diagonal gathered over the mailbox: 3 ranks on one GPU; the
    worker compares all n entries on every rank and checks its plan, its rank count and the reported rel_residual."""
    out = tmp_path / "p2p_scaled.txt"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "3", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", worker), "3000", "80", str(out), str(tagged), "scaled"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=420, env=dict(os.environ, OMP_NUM_THREADS="1", MASTER_ADDR="127.0.0.1"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert open(out).read().strip() == "same bits", open(out).read()


# ---- 1f. a second matrix on one context --------------------------------------------------------------------------------------
def _write_mtx(path, A):
    i, j = np.nonzero(A)
    with open(path, "w") as f:
        f.write("%%%%MatrixMarket matrix coordinate real general\n%d %d %d\n" % (A.shape[0], A.shape[1], len(i)))
        f.writelines("%d %d %r\n" % (a + 1, b + 1, float(v)) for a, b, v in zip(i, j, A[i, j]))   # repr: every double exactly
    return str(path)


@pytest.mark.parametrize("storage,how", [("dense", "set_matrix_dense"), ("dense", "read_matrix"), ("csr", "set_matrix_csr"),
                                         ("csr", "read_matrix")])
def test_second_matrix_on_one_context_gets_its_own_diagonal(gpu_pkg, oracle, tmp_path, storage, how):
    """dinv_valid: Jacobi on S1 L S1, a new matrix S2 L S2 of the same size, Jacobi again -- the second x is S2^-1 x~ bit for
    bit, so nothing of S1's diagonal is left.  Then the preconditioner off and on again without a new matrix."""
    n, iters = 1024, 60
    L = oracle.generate_lap2d(n)
    s1, s2 = _scale(n, 1), _scale(n, 2)
    assert np.count_nonzero(s1 != s2) > n // 2
    bt = oracle.init_source_term(n)
    mats = {"L": L, "1": _sls_dense(L, s1), "2": _sls_dense(L, s2)}
    files = {k: _write_mtx(tmp_path / (k + ".mtx"), A) for k, A in mats.items()} if how == "read_matrix" else {}
    fmt = gpu_pkg.MATRIX_CSR if storage == "csr" else gpu_pkg.MATRIX_DENSE
    want = 7 if storage == "csr" else 1

    def load(c, key):
        if how == "read_matrix":
            c.read_matrix(files[key])
        elif how == "set_matrix_csr":
            c.set_matrix_csr(*tc.dense_to_csr(mats[key]))
        else:
            c.set_matrix_dense(mats[key])
        assert c.gemv_plan()["variant"] == want and _shards(c) == 1, c.gemv_plan()
        assert np.array_equal(c.probe_matrix_rows(0)[0], mats[key])

    with gpu_pkg.CGSolver(matrix_format=fmt, gemv_variant=-1) as c:
        load(c, "L")
        xt, _ = _solve(c, bt, iters, False)
    with gpu_pkg.CGSolver(matrix_format=fmt, gemv_variant=-1) as c:
        load(c, "2")
        xp2, _ = _solve(c, s2 * bt, iters, False)          # plain CG on S2 L S2, a fresh context
    with gpu_pkg.CGSolver(matrix_format=fmt, gemv_variant=-1) as c:
        load(c, "1")
        x1, r1 = _solve(c, s1 * bt, iters, True)
        load(c, "2")
        x2, r2 = _solve(c, s2 * bt, iters, True)
        xoff, _ = _solve(c, s2 * bt, iters, False)          # off ...
        x3, r3 = _solve(c, s2 * bt, iters, True)            # ... and on again, no new matrix
        assert c.gemv_plan()["variant"] == want
    _assert_same_bits(s1, x1, xt, "first matrix")
    _assert_same_bits(s2, x2, xt, "second matrix")
    _assert_same_bits(np.ones(n), xoff, xp2, "preconditioner off")
    _assert_same_bits(s2, x3, xt, "preconditioner on again")
    for key, s, x, r in (("1", s1, x1, r1), ("2", s2, x2, r2), ("2", s2, x3, r3)):
        ax, aax = _dense_products(mats[key], x)
        _check_rel_residual(r, ax, aax, s * bt, 5, key)


# ---- 2. diagonals that are not powers of two, against the longdouble PCG -------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _sls_reference():
    """tests/test_gpu_jacobi.py's matrix and longdouble references: x after 60 iterations, and the run to tol = 1e-6 ||b||."""
    import __graft_entry__ as g
    O = g.load_oracle()
    _, A = tj._sls(O)
    b = O.init_source_term(tj.N_SLS)
    x60, k60 = tj._pcg_longdouble(A, b, 60)
    assert k60 == 60
    tol = tj._tol(O)
    _, kref = tj._pcg_longdouble(A, b, tj.N_SLS, tol)
    assert kref == tj.K_JACOBI_SLS
    return A, b, x60, tol, kref, tj._pcg_longdouble.residual_prev


def _against_longdouble(pkg, check_plan, what, **kw):
    A, b, x60, tol, kref, prev = _sls_reference()
    n = len(b)
    with pkg.CGSolver(**kw) as c:
        c.set_matrix_dense(A)
        c.set_preconditioner("jacobi")
        check_plan(c)
        x, res = _solve(c, b, 60, True)
        err = np.linalg.norm(x - x60) / np.linalg.norm(x60)
        print("longdouble %r: |x - x_ref| / |x_ref| = %.3e" % (what, err))
        assert err <= tj.REL_BOUND, (what, err)
        ax, aax = _dense_products(A, x)
        _check_rel_residual(res, ax, aax, b, 5, what)
        x, res = _solve(c, b, n, True, tol)
        check_plan(c)
    print("longdouble %r: stops at %d (reference %d), residual_prev %.17g (reference %.17g)" % (
        what, res["iterations"], kref, res["residual_prev"], prev))
    assert res["converged"] == 1 and res["iterations"] == kref == tj.K_JACOBI_SLS, (what, res)
    assert res["residual_last"] < tol <= res["residual_prev"], res
    assert abs(res["residual_prev"] - prev) <= 1e-9 * prev, (what, res, prev)
    ax, aax = _dense_products(A, x)
    _check_rel_residual(res, ax, aax, b, 5, what)


@pytest.mark.parametrize("p", [2, 3, 8])
def test_loopback_shards_nonuniform_diagonal_against_longdouble(gpu_pkg, p):
    _against_longdouble(gpu_pkg, _loopback_check(gpu_pkg, p), p, comm_mode=gpu_pkg.COMM_LOOPBACK, nranks=p)


@pytest.mark.parametrize("variant", [10822, 10442, 10444, 10445])
def test_one_round_shapes_nonuniform_diagonal_against_longdouble(gpu_pkg, variant):
    _against_longdouble(gpu_pkg, _shape_check(variant), variant, gemv_variant=variant)


def _pcg_longdouble_with_residual(A, b, iters):
    """tests/test_gpu_jacobi.py _pcg_longdouble at tol = 0, returning also sqrt(r.r) as the CLI prints it after a loop that ran
    out: rsold = rsnew of the last iteration (cg.cc:132), i.e. after the last update."""
    A = A.astype(np.longdouble)
    b = b.astype(np.longdouble)
    dinv = 1 / np.diag(A)
    x = np.zeros_like(b)
    r = b.copy()
    z = dinv * r
    p = z.copy()
    rho = r @ z
    for _ in range(iters):
        Ap = A @ p
        alpha = rho / (p @ Ap)
        x += alpha * p
        r -= alpha * Ap
        z = dinv * r
        rn = r @ z
        p = z + (rn / rho) * p
        rho = rn
    return x.astype(np.float64), float(np.sqrt(r @ r))


@pytest.fixture(scope="module")
def sls_file(gpu_pkg, oracle, tmp_path_factory):
    """S L S with s spread over [1, 100] as a Matrix-Market file, and the longdouble PCG of the matrix the library's own parser
    makes of that file: (path, ||x||, printed residual) after 60 iterations."""
    n, iters = tj.N_SLS, 60
    _, A = tj._sls(oracle)
    path = _write_mtx(tmp_path_factory.mktemp("sls") / "sls.mtx", A)
    m, nn, sym, I, J, a = gpu_pkg.cgx.parse_matrix_market(path)
    assert (m, nn, sym) == (n, n, False)
    Af = np.zeros((n, n))
    Af[I, J] = a
    assert np.array_equal(Af, A)
    b = oracle.init_source_term(n)
    xr, res_ref = _pcg_longdouble_with_residual(Af, b, iters)
    assert np.array_equal(xr, tj._pcg_longdouble(Af, b, iters)[0])   # the same recurrence as the imported reference
    return path, iters, float(np.linalg.norm(xr.astype(np.longdouble))), res_ref


RCCL = ["--gpus", "2", "--same-device", "--transport", "rccl"]


@pytest.mark.parametrize("name,extra", [("rccl dense", RCCL), ("rccl csr", RCCL + ["--csr"]), ("loopback dense", ["--loopback", "2"])],
                         ids=["rccl-dense", "rccl-csr", "loopback-dense"])
def test_cli_transports_nonuniform_diagonal_against_longdouble(gpu_pkg, fake_rccl_dir, sls_file, tmp_path, name, extra):  # noqa: F811
    """`cgsolver FILE OUT 60 --jacobi` on S L S: the RCCL transport (test double, two processes on one GPU) on dense and CSR
    storage, and two loopback shards.  The printed ||x|| and residual against the longdouble PCG: 2e-6 relative, what seven
    printed digits allow (the bar of tests/test_gpu_rccl_path.py).  The transports fold in different orders, so the lines are
    not compared with each other."""
    path, iters, xn_ref, res_ref = sls_file
    env = dict(os.environ, LD_LIBRARY_PATH=fake_rccl_dir + os.pathsep + os.environ.get("LD_LIBRARY_PATH", ""))
    r = subprocess.run([EXE, path, str(tmp_path / "out"), str(iters)] + extra + ["--jacobi", "--stats"], capture_output=True,
                       text=True, timeout=300, env=env)
    assert r.returncode == 0, (name, r.stdout[-2000:], r.stderr[-2000:])
    if "rccl" in name:
        assert "fake_rccl: rank 1 of 2 wired" in r.stderr, r.stderr[-2000:]
    stats = re.search(r"cgsolver stats: .*", r.stderr).group(0)
    assert stats.endswith("precond=jacobi") and " gpus=2 " in stats and " loop=per-launch" in stats, stats
    assert ("format=csr" in stats) == ("csr" in name), stats
    mm = re.search(r"\[STEP (\d+)\] residual = (\S+), \|\|x\|\| = (\S+),", r.stdout)
    assert mm, r.stdout
    k, res, xn = int(mm.group(1)), float(mm.group(2)), float(mm.group(3))
    print("cli %s: k=%d residual %.6e (reference %.9e) ||x|| %.6e (reference %.9e)" % (name, k, res, res_ref, xn, xn_ref))
    assert k == iters
    assert abs(xn - xn_ref) <= 2e-6 * xn_ref, (name, xn, xn_ref)
    assert abs(res - res_ref) <= 2e-6 * res_ref, (name, res, res_ref)
