"""The symmetric K1 (plan variant 6, csrc/cgx_symv.hip): A p from the upper triangle of an exactly symmetric A on one GPU.

Selection follows an exact (bitwise) symmetry check that runs behind every writer of A; explicit shapes, several shards and
banded storage keep the general kernels.  The product is checked on sampled rows of dense hash matrices at uneven n against
the rows rebuilt on the host, within the summation-order bound of tests/test_gpu_dense_hash.py, and whole solves against
the oracle.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 0x5EEDC0DE
B = 256   # tile edge of the symmetric kernel (cgx_kernels.h kSymvTile)


def _diag(n):
    return 1.03 * 2.0 * np.sqrt(n / 3.0)   # SPD hash matrix (tests/test_gpu_dense_hash.py)


@pytest.mark.parametrize("n,want", [(16385, 6), (20001, 6), (32768, 6), (16384, 1)])
def test_generated_matrix_selects_the_symmetric_kernel_above_16384(gpu_pkg, n, want):
    with gpu_pkg.CGSolver(gemv_variant=-1) as s:
        s.generate_lap2d_matrix(n)
        plan = s.gemv_plan()
    assert plan["variant"] == want, plan
    if want == 6:
        nb = (n + B - 1) // B
        sr = (n + 1) // 2 * 2
        assert plan["R"] == B and plan["split"] == nb and plan["light"] == (sr + 127) // 128, plan


@pytest.mark.parametrize("kw,want", [(dict(gemv_variant=10821), 1), ("loopback", 1), ("banded", 3)])
def test_explicit_shape_shards_and_banded_storage_keep_their_kernels(gpu_pkg, kw, want):
    n = 20001
    if kw == "loopback":
        kw = dict(comm_mode=gpu_pkg.COMM_LOOPBACK, nranks=2)
    elif kw == "banded":
        kw = dict(matrix_format=gpu_pkg.MATRIX_BANDED)
    with gpu_pkg.CGSolver(**kw) as s:
        s.generate_lap2d_matrix(n)
        assert s.gemv_plan()["variant"] == want


def test_plan_follows_every_rewrite_of_the_matrix(gpu_pkg):
    n = 20001
    with gpu_pkg.CGSolver() as s:
        s.generate_lap2d_matrix(n)
        s.probe_fill_matrix_hash(SEED, symmetric=True)
        assert s.gemv_plan()["variant"] == 6
        s.probe_fill_matrix_hash(SEED, symmetric=False)
        assert s.gemv_plan()["variant"] == 1
        s.probe_fill_matrix_hash(SEED, symmetric=True)
        assert s.gemv_plan()["variant"] == 6


def _one_ulp_asymmetric(oracle, n):
    A = oracle.hash_rows(n, 0, n, SEED + 7, True, _diag(n))
    A[3, n - 2] = np.nextafter(A[3, n - 2], np.inf)
    return A


def test_one_ulp_off_symmetry_keeps_the_general_kernel_and_solves(gpu_pkg, oracle):
    """set_matrix_dense of a symmetric matrix with ONE element moved by one ulp: the general K1, and three CG iterations on
    exactly that matrix match oracle.solve on it."""
    n, iters = 16500, 3
    A = _one_ulp_asymmetric(oracle, n)
    with gpu_pkg.CGSolver() as s:
        s.set_matrix_dense(A)
        assert s.gemv_plan()["variant"] == 1
        s.init_source_term(1.0 / n)
        s.set_max_iter(iters)
        s.tolerance(0.0)
        x = np.zeros(n)
        r = s.solve(x)
        A[3, n - 2] = A[n - 2, 3]   # and back to symmetric: the plan follows
        s.set_matrix_dense(A)
        assert s.gemv_plan()["variant"] == 6
    A[3, n - 2] = np.nextafter(A[3, n - 2], np.inf)
    oracle.set_threads(16)
    try:
        xo, ro = oracle.solve(A, oracle.init_source_term(n), max_iter=iters, tol=0.0)
    finally:
        oracle.set_threads(1)
    assert r["iterations"] == ro["iterations"] == iters
    assert np.linalg.norm(x - xo) <= 1e-12 * np.linalg.norm(xo)


def _crossing_rows(n, lda):
    out, k = [], 1
    while True:
        r = (k << 32) // (lda * 8)
        if r >= n:
            break
        out += [x for x in range(r - 3, r + 4) if 0 <= x < n]
        k += 1
    return out


@pytest.mark.parametrize("n", [16385, 20001, 23170, 46340])
def test_symmetric_gemv_on_dense_hash_matrices(gpu_pkg, oracle, n):
    """cgx_probe_gemv through the symmetric kernel: >= 256 sampled rows -- first and last row of every 256-row block, the rows
    next to 4 GiB offsets, random others -- against the rows rebuilt on the host; and the fused p.Ap."""
    rng = np.random.default_rng(n)
    pv = rng.standard_normal(n)
    with gpu_pkg.CGSolver() as s:
        s.generate_lap2d_matrix(n)
        s.probe_fill_matrix_hash(SEED + n, symmetric=True)
        plan = s.gemv_plan()
        assert plan["variant"] == 6, plan
        y, pap = s.probe_gemv(pv)
    lda = (n + 15) // 16 * 16 + 16
    rows = set()
    for b0 in range(0, n, B):
        rows |= {b0, min(b0 + B, n) - 1}
    rows |= set(_crossing_rows(n, lda))
    rows |= set(int(v) for v in rng.integers(0, n, size=200))
    rows = sorted(r for r in rows if 0 <= r < n)
    assert len(rows) >= 256
    for i0 in range(0, len(rows), 64):
        idx = rows[i0:i0 + 64]
        A = np.vstack([oracle.hash_rows(n, r, 1, SEED + n, True, 0.0) for r in idx])
        yo = oracle.gemv(A, pv)
        bound = 4e-16 * np.sqrt(n) * (np.abs(A) @ np.abs(pv))
        err = np.abs(y[idx] - yo)
        assert np.all(err <= bound), (plan, [(r, e, b) for r, e, b in zip(idx, err, bound) if e > b][:4])
    assert np.all(np.isfinite(y))
    assert abs(pap - float(np.dot(pv, y))) <= 1e-12 * float(np.sum(np.abs(pv * y)))


def test_200_iterations_at_n20001_against_the_oracle(gpu_pkg, oracle):
    n, iters = 20001, 200
    with gpu_pkg.CGSolver() as s:
        s.generate_lap2d_matrix(n)
        assert s.gemv_plan()["variant"] == 6
        s.init_source_term(1.0 / n)
        s.set_max_iter(iters)
        x = np.zeros(n)
        r = s.solve(x)
    xo, ro = oracle.solve_lap2d_banded(n, iters, 1e-10, 1)
    assert r["iterations"] == ro["iterations"] == iters
    assert np.linalg.norm(x - xo) <= 1e-12 * np.linalg.norm(xo)


def test_solves_are_bitwise_reproducible(gpu_pkg):
    n, iters = 20001, 50

    def run(s):
        s.generate_lap2d_matrix(n)
        s.probe_fill_matrix_hash(SEED + 3, symmetric=True, diag=_diag(n))
        assert s.gemv_plan()["variant"] == 6
        s.init_source_term(1.0 / n)
        s.set_max_iter(iters)
        s.tolerance(0.0)
        x = np.zeros(n)
        s.solve(x)
        return x

    with gpu_pkg.CGSolver() as s:
        a = run(s)
        b = run(s)
    with gpu_pkg.CGSolver() as s:
        c = run(s)
    assert np.array_equal(a, b) and np.array_equal(a, c)
