"""The symmetric K1 (plan variant 6, csrc/cgx_symv.hip) against high-precision references on dense data.

tests/test_gpu_symmetric.py checks sampled rows of the plain product against a double sum and whole solves on
generate_lap2d, whose far tiles are zero.  Here:
  - every row of the plain product (probe_gemv) on dense symmetric hash matrices against y = A p summed in np.longdouble
    (oracle.hash_gemv_longdouble), within the suite's summation-order bound, and p.Ap against p.(A p) from the same sums;
  - the fused tile kernel (beta applied on the fly, transposed column pieces of far tiles) through whole solves on a dense SPD
    hash matrix against oracle.solve, which sees every row of A p from the second iteration on;
  - the early return of the tile kernel and the `done` predicate of the fold (convergence before max_iter), the p[k & 1] parity
    across solve_steps calls, a nonzero x0 through the plain product, and solves on both sides of plan switches;
  - the bit-for-bit symmetry check at the edges of its 32 x 32 tiles and on late grid-stride passes;
  - a symmetric Matrix-Market file large enough for variant 6.
Every test asserts the plan it means to run, so a later plan change cannot make it test another kernel.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 0x51A7E5
B = 256   # tile edge of the symmetric kernel (cgx_kernels.h kSymvTile)


def _diag(n):
    return 1.03 * 2.0 * np.sqrt(n / 3.0)   # SPD hash matrix (tests/test_gpu_dense_hash.py)


def _rhs(n):
    return np.random.default_rng(n + 1).standard_normal(n)


_HOST = {}   # one full host copy of an SPD hash matrix at a time (2.1 GB at n = 16385), shared by the solve tests


def _host_spd(oracle, n, seed):
    key = (n, seed)
    if key not in _HOST:
        _HOST.clear()
        oracle.set_threads(16)
        try:
            _HOST[key] = oracle.hash_rows(n, 0, n, seed, True, _diag(n))
        finally:
            oracle.set_threads(1)
    return _HOST[key]


def _oracle_solve(oracle, A, b, iters, tol=0.0, x0=None):
    return oracle.solve(A, b, x0=x0, max_iter=iters, tol=tol)


def _close(x, xo, r, ro, rtol_res=1e-11):
    assert r["iterations"] == ro["iterations"]
    assert np.linalg.norm(x - xo) <= 1e-12 * np.linalg.norm(xo), np.linalg.norm(x - xo) / np.linalg.norm(xo)
    assert abs(r["residual_prev"] - ro["residual_prev"]) <= rtol_res * ro["residual_prev"], (r, ro)


# ---- the plain product, every row ---------------------------------------------------------------------------------------------
def _ranges(rows):
    """Sorted row indices as (row0, nrows) runs."""
    out = []
    for r in rows:
        if out and out[-1][0] + out[-1][1] == r:
            out[-1][1] += 1
        else:
            out.append([r, 1])
    return [tuple(v) for v in out]


def _gemv_through_variant6(gpu_pkg, n, seed, pv):
    with gpu_pkg.CGSolver() as s:
        s.generate_lap2d_matrix(n)
        s.probe_fill_matrix_hash(seed, symmetric=True)
        plan = s.gemv_plan()
        assert plan["variant"] == 6, plan
        y, pap = s.probe_gemv(pv)
    assert np.all(np.isfinite(y))
    return plan, y, pap


def _assert_rows(oracle, n, plan, y, rows, yr, abs_ap):
    bad = oracle.gemv_rows_outside(y[rows], yr, abs_ap, n)
    bound = 4e-16 * np.sqrt(n) * abs_ap
    assert bad.size == 0, (plan, bad.size, [(int(rows[i]), float(abs(y[rows[i]] - yr[i])), float(bound[i])) for i in bad[:6]])


@pytest.mark.parametrize("n", [16385, 16512, 16639, 16640, 20001])   # n mod 256 = 1, 128, 255, 0, 33
def test_every_row_of_the_symmetric_product_and_pap(gpu_pkg, oracle, n):
    """probe_gemv through variant 6 on a dense symmetric hash matrix: every row against the longdouble product, and the fused
    p.Ap against p.(A p) within the row bounds carried through plus the rounding of an n-term dot."""
    seed = SEED + n
    pv = np.random.default_rng(n).standard_normal(n)
    plan, y, pap = _gemv_through_variant6(gpu_pkg, n, seed, pv)
    oracle.set_threads(16)
    try:
        rows, yr, abs_ap = oracle.hash_gemv_longdouble(n, seed, pv, symmetric=True)
    finally:
        oracle.set_threads(1)
    _assert_rows(oracle, n, plan, y, rows, yr, abs_ap)
    pap_ref = np.sum(pv.astype(np.longdouble) * yr)
    tol = np.sum(np.abs(pv) * 4e-16 * np.sqrt(n) * abs_ap) + 4e-16 * np.sqrt(n) * np.sum(np.abs(pv * y))
    assert abs(pap - pap_ref) <= tol, (plan, float(pap - pap_ref), float(tol))


def test_symmetric_product_at_the_bench_size(gpu_pkg, oracle):
    """n = 32768 = 128 blocks (no partial block): every row of blocks 0, 1, nb/2 and nb - 1, the first and last row of every
    block, and random rows, against the longdouble product."""
    n = 32768
    nb = n // B
    seed = SEED + n
    rng = np.random.default_rng(n)
    pv = rng.standard_normal(n)
    plan, y, pap = _gemv_through_variant6(gpu_pkg, n, seed, pv)
    rows = set()
    for blk in (0, 1, nb // 2, nb - 1):
        rows |= set(range(blk * B, (blk + 1) * B))
    for b0 in range(0, n, B):
        rows |= {b0, b0 + B - 1}
    rows |= set(int(v) for v in rng.integers(0, n, size=200))
    oracle.set_threads(16)
    try:
        rr, yr, abs_ap = oracle.hash_gemv_longdouble(n, seed, pv, symmetric=True, ranges=_ranges(sorted(rows)))
    finally:
        oracle.set_threads(1)
    assert rr.size == len(rows) >= 4 * B + 2 * nb
    _assert_rows(oracle, n, plan, y, rr, yr, abs_ap)
    assert abs(pap - float(np.dot(pv, y))) <= 1e-12 * float(np.sum(np.abs(pv * y)))


# ---- the fused tile kernel ---------------------------------------------------------------------------------------------------
def _spd_context(gpu_pkg, n, seed, **kw):
    s = gpu_pkg.CGSolver(**kw)
    s.generate_lap2d_matrix(n)
    s.probe_fill_matrix_hash(seed, symmetric=True, diag=_diag(n))
    assert s.gemv_plan()["variant"] == 6
    s.set_source_term(_rhs(n))
    return s


@pytest.mark.parametrize("n", [16385, 16640])
def test_fused_tile_kernel_against_the_oracle(gpu_pkg, oracle, n):
    """1, 2, 3 and 40 CG iterations on a dense SPD hash matrix: from the second iteration on x carries every row of A p of the
    fused kernel (p = r + beta p_old formed in the tile kernel, far tiles used transposed)."""
    seed = SEED + 2 * n
    out = {}
    with _spd_context(gpu_pkg, n, seed) as s:
        s.tolerance(0.0)
        for iters in (1, 2, 3, 40):
            s.set_max_iter(iters)
            x = np.zeros(n)
            out[iters] = (x, s.solve(x))
    A, b = _host_spd(oracle, n, seed), _rhs(n)
    for iters, (x, r) in out.items():
        xo, ro = _oracle_solve(oracle, A, b, iters)
        assert r["iterations"] == iters
        _close(x, xo, r, ro, 1e-11 if iters <= 3 else 1e-8)
        assert abs(r["rel_residual"] - ro["rel_residual"]) <= 1e-9 * ro["rel_residual"]


# ---- convergence, break and stepping -----------------------------------------------------------------------------------------
N_STEP = 16640   # n mod 256 = 0: the stepping tests' size


def test_convergence_before_max_iter_and_no_updates_after_the_break(gpu_pkg, oracle):
    """tol between two consecutive oracle residuals, far from both: the same iteration count as the oracle, converged, and x
    close to the oracle's.  Iterations enqueued past the break (check_every 64, and steps of one solve_steps call beyond it)
    leave x bitwise what the host-checked run (check_every 1) gives: the tile kernel's early return and the fold's `done`."""
    n, seed, K = N_STEP, SEED + 2 * N_STEP, 20
    A, b = _host_spd(oracle, n, seed), _rhs(n)
    _, rk = _oracle_solve(oracle, A, b, K)
    tol = 1.1 * rk["residual_last"]
    xo, ro = _oracle_solve(oracle, A, b, 200, tol=tol)
    assert ro["converged"] and ro["iterations"] <= K
    assert ro["residual_last"] < tol / 1.05 and ro["residual_prev"] > 1.05 * tol, (ro, tol)

    xs = []
    for every in (1, 64):
        with _spd_context(gpu_pkg, n, seed, check_every=every) as s:
            s.set_max_iter(200)
            s.tolerance(tol)
            x = np.zeros(n)
            r = s.solve(x)
        assert r["converged"], r
        _close(x, xo, r, ro, 1e-9)
        assert abs(r["residual_last"] - ro["residual_last"]) <= 1e-9 * ro["residual_last"]
        xs.append((x, r))
    assert np.array_equal(xs[0][0], xs[1][0]) and xs[0][1]["residual_prev"] == xs[1][1]["residual_prev"]

    with _spd_context(gpu_pkg, n, seed, check_every=64) as s:
        s.set_max_iter(200)
        s.tolerance(tol)
        s.solve_begin(np.zeros(n))
        assert s.solve_steps(ro["iterations"] + 30)
        assert s.solve_steps(7)
        x = np.zeros(n)
        r = s.solve_end(x)
    assert r["converged"] and r["iterations"] == ro["iterations"]
    assert np.array_equal(x, xs[0][0])


def test_steps_of_1_5_31_equal_one_37_iteration_solve(gpu_pkg):
    """bench.py's path: solve_begin / solve_steps / solve_end, with p[k & 1] carried across calls of odd and even lengths."""
    n, seed = N_STEP, SEED + 2 * N_STEP
    with _spd_context(gpu_pkg, n, seed) as s:
        s.set_max_iter(37)
        s.tolerance(0.0)
        x1 = np.zeros(n)
        r1 = s.solve(x1)
        s.solve_begin(np.zeros(n))
        for k in (1, 5, 31):
            assert not s.solve_steps(k)
        x2 = np.zeros(n)
        r2 = s.solve_end(x2)
        assert s.gemv_plan()["variant"] == 6
    assert r1["iterations"] == r2["iterations"] == 37
    assert np.array_equal(x1, x2)
    assert r1["residual_prev"] == r2["residual_prev"] and r1["rel_residual"] == r2["rel_residual"]


def test_nonzero_initial_guess_through_the_plain_product(gpu_pkg, oracle):
    """r0 = b - A x0 and the verification product (rel_residual) both go through the plain symmetric product."""
    n, seed, iters = N_STEP, SEED + 2 * N_STEP, 10
    x0 = 0.05 * np.random.default_rng(5).standard_normal(n)
    with _spd_context(gpu_pkg, n, seed) as s:
        s.set_max_iter(iters)
        s.tolerance(0.0)
        s.solve_begin(x0)
        s.solve_steps(iters)
        x = np.zeros(n)
        r = s.solve_end(x)
    A, b = _host_spd(oracle, n, seed), _rhs(n)
    xo, ro = _oracle_solve(oracle, A, b, iters, x0=x0)
    assert r["iterations"] == iters
    _close(x, xo, r, ro, 1e-10)
    assert abs(r["rel_residual"] - ro["rel_residual"]) <= 1e-9 * ro["rel_residual"]
    assert abs(r["x_norm"] - ro["x_norm"]) <= 1e-12 * ro["x_norm"]


# ---- plan switches with solves in between ------------------------------------------------------------------------------------
def test_solves_across_plan_switches(gpu_pkg, oracle):
    """6 -> 1 -> 6 on one context (the partial count K3 folds changes, the slot buffer is reused), a solve on each matrix
    against the oracle on exactly that matrix."""
    n, seed, iters = 16385, SEED + 2 * 16385, 5
    A, b = _host_spd(oracle, n, seed), _rhs(n)
    i, j = 4000, n - 7
    a_ij = A[i, j]
    xs = []
    with gpu_pkg.CGSolver() as s:
        s.generate_lap2d_matrix(n)
        for step, want in enumerate((6, 1, 6)):
            if step == 0:
                s.probe_fill_matrix_hash(seed, symmetric=True, diag=_diag(n))
            else:
                A[i, j] = np.nextafter(a_ij, np.inf) if want == 1 else a_ij
                try:
                    s.set_matrix_dense(A)
                finally:
                    A[i, j] = a_ij
            assert s.gemv_plan()["variant"] == want
            s.set_source_term(b)
            s.set_max_iter(iters)
            s.tolerance(0.0)
            x = np.zeros(n)
            xs.append((x, s.solve(x)))
    xo, ro = _oracle_solve(oracle, A, b, iters)
    A[i, j] = np.nextafter(a_ij, np.inf)
    try:
        xo1, ro1 = _oracle_solve(oracle, A, b, iters)
    finally:
        A[i, j] = a_ij
    _close(xs[0][0], xo, xs[0][1], ro)
    _close(xs[1][0], xo1, xs[1][1], ro1)
    _close(xs[2][0], xo, xs[2][1], ro)
    assert np.array_equal(xs[0][0], xs[2][0])


# ---- the symmetry check at its edges -----------------------------------------------------------------------------------------
def _pair_index(i, j, n):
    """Index of the 32 x 32 tile pair that compares (i, j) with (j, i) in k_symmetric_check's walk (tri_tile order)."""
    nt = (n + 31) // 32
    I, J = sorted((i // 32, j // 32))
    return I * nt - I * (I - 1) // 2 + (J - I)


@pytest.mark.parametrize("n", [16385, 16400])   # n mod 32 = 1, 16
def test_symmetry_check_at_tile_edges(gpu_pkg, oracle, n):
    """One element moved by one ulp -- in the upper and in the lower element of each pair -- plans the general K1; put back it
    plans variant 6 again.  +0.0 against -0.0 is a difference (the bit-for-bit contract of include/cgx.h)."""
    _HOST.clear()
    oracle.set_threads(16)
    try:
        A = oracle.hash_rows(n, 0, n, SEED + 3 * n, True, _diag(n))
    finally:
        oracle.set_threads(1)
    positions = [
        (1, 0),            # diagonal check tile
        (n - 1, n - 2),    # last (partial) diagonal check tile
        (0, n - 1),        # corner
        (31, 32),          # across a check-tile boundary
        (n - 1, n - 33),   # a pair on a late grid-stride pass
    ]
    assert _pair_index(n - 1, n - 33, n) >= 8192   # launch_symmetric_check: grid of at most 8192 workgroups
    with gpu_pkg.CGSolver() as s:
        s.set_matrix_dense(A)
        assert s.gemv_plan()["variant"] == 6
        for i, j in positions:
            for a, c in ((i, j), (j, i)):
                old = A[a, c]
                A[a, c] = np.nextafter(old, np.inf)
                try:
                    s.set_matrix_dense(A)
                finally:
                    A[a, c] = old
                assert s.gemv_plan()["variant"] == 1, (n, a, c)
                s.set_matrix_dense(A)
                assert s.gemv_plan()["variant"] == 6, (n, a, c)
        d = A[5, 5]                                   # the diagonal has no partner: still symmetric
        A[5, 5] = np.nextafter(d, np.inf)
        try:
            s.set_matrix_dense(A)
            assert s.gemv_plan()["variant"] == 6
        finally:
            A[5, 5] = d
        i, j = 5, n - 40
        old = A[i, j]
        try:
            A[i, j], A[j, i] = 0.0, -0.0
            s.set_matrix_dense(A)
            assert s.gemv_plan()["variant"] == 1
            A[j, i] = 0.0
            s.set_matrix_dense(A)
            assert s.gemv_plan()["variant"] == 6
        finally:
            A[i, j] = A[j, i] = old
        s.set_matrix_dense(A)
        assert s.gemv_plan()["variant"] == 6


# ---- Matrix-Market input -----------------------------------------------------------------------------------------------------
def _mtx_entries(g, couplings, seed):
    """A 5-point Laplacian on a g x g grid plus `couplings` random symmetric entries at least 1024 columns off the diagonal,
    with the diagonal raised above each row's absolute sum (SPD).  Returns {(i, j): a} for i >= j."""
    n = g * g
    rng = np.random.default_rng(seed)
    lower = {}
    for i in range(n):
        if i % g:
            lower[(i, i - 1)] = -1.0
        if i >= g:
            lower[(i, i - g)] = -1.0
    while len(lower) < 2 * n - 2 * g + couplings:
        i, j = (int(v) for v in rng.integers(0, n, size=2))
        if i - j >= 1024:
            lower[(i, j)] = float(rng.uniform(-1.0, 1.0))
    rowsum = np.zeros(n)
    for (i, j), a in lower.items():
        rowsum[i] += abs(a)
        rowsum[j] += abs(a)
    for i in range(n):
        lower[(i, i)] = 1.0 + rowsum[i]
    return lower


def _write_mtx(path, n, kind, entries):
    with open(path, "w") as f:
        f.write("%%%%MatrixMarket matrix coordinate real %s\n%d %d %d\n" % (kind, n, n, len(entries)))
        f.writelines("%d %d %r\n" % (i + 1, j + 1, float(a)) for (i, j), a in entries)


def test_matrix_market_input_into_variant6(gpu_pkg, oracle, tmp_path):
    """A symmetric coordinate file with n = 16641 (129^2, lower triangle only) plans variant 6 and solves as the oracle does
    on the same file; the general file with every entry and one of them moved by one ulp plans the general K1."""
    _HOST.clear()
    g, iters = 129, 30
    n = g * g
    lower = _mtx_entries(g, 3000, n)
    far = [(i, j) for (i, j) in lower if i - j >= 1024]
    assert len(far) == 3000 and len({(i // B, j // B) for i, j in far}) > 1000   # far tiles are non-zero
    sym = tmp_path / "sym.mtx"
    _write_mtx(sym, n, "symmetric", sorted(lower.items()))
    full = dict(lower)
    full.update({(j, i): a for (i, j), a in lower.items() if i != j})
    i0, j0 = far[0]
    full[(j0, i0)] = float(np.nextafter(full[(j0, i0)], np.inf))
    gen = tmp_path / "gen.mtx"
    _write_mtx(gen, n, "general", sorted(full.items()))
    b = _rhs(n)
    for path, want in ((sym, 6), (gen, 1)):
        with gpu_pkg.CGSolver() as s:
            s.read_matrix(str(path))
            assert s.gemv_plan()["variant"] == want, path
            s.set_source_term(b)
            s.set_max_iter(iters)
            s.tolerance(0.0)
            x = np.zeros(n)
            r = s.solve(x)
        A, _, is_sym = oracle.read_mtx_dense(str(path))
        assert is_sym == (want == 6) and np.array_equal(A, A.T) == (want == 6)
        xo, ro = _oracle_solve(oracle, A, b, iters)
        del A
        assert r["iterations"] == iters
        _close(x, xo, r, ro, 1e-9)
