"""The Lanczos family (cgx_lanczos, cgx_trace_slq, cgx_apply_function, cgx_eigenpairs and their probes: csrc/cgx_lanczos.hip,
csrc/cgx_funm.hip, csrc/cgx_eigs.hip, the multi-vector K1 of csrc/cgx_multi.hip) past 16 row tiles and past 256 K1 partials.

test_gpu_lanczos.py, test_gpu_funm.py and test_gpu_eigs.py compare with references at n <= 1024: at most 4 tiles of 256 rows and
at most 128 partials of p.Ap per column, so that neither the 16-tile trips of k_eigs_subtract's fold of h nor any slot but the first
of fold_pap (csrc/cgx_device.h: four clamped loads per thread at f + 256 u, the loop going on in steps of 1024) has run there.
Here, with tiles = ceil(n / 256) (the step kernels' grid g3 and the tile partials they fold) and g1 = the workgroups of K1m, one
p.Ap partial each per column (64 rows per workgroup at the widths 1, 2 and 4, 32 at width 8, 8 at width 16):

      n    matrix  tiles  g1 at width 1,2,4 / 8 / 16   fold of h (16 tiles per trip)   fold_pap over g1 at width 16
   4096    hash      16       64 /  128 /  512         1 trip, no tail                 slots 0, 1 (full)
   4100    hash      17       65 /  129 /  513         1 trip and a tail of 1          slots 0, 1 and one partial in slot 2
   7937    hash      32      125 /  249 /  993         2 trips, no tail                slots 0 .. 3 (the pass alone runs here)
   8200    lap2d     33      129 /  257 / 1025         2 trips and a tail of 1         slots 0 .. 3 and one partial in a 2nd trip
  16400    lap2d     65      257 /  513 / 2050         4 trips and a tail of 1         two trips and two partials in a third

(g1 = 257 -- one partial in slot 1 -- is width 8 at n = 8200 and the widths 1, 2, 4 at n = 16400.)  The last tile holds 4 rows at
n = 4100, 1 at 7937, 8 at 8200 and 16 at 16400; none at 4096.

1. cgx_lanczos: the coefficients against the longdouble recurrence (test_gpu_lanczos's check), no breakdown in the float64
   restatement, the width rule of include/cgx.h and reversed columns bit for bit;
2. breakdown beside running columns at 17 tiles (test_gpu_lanczos's scenario);
3. cgx_trace_slq at 65 tiles: per probe the quadrature of the device's own coefficients;
4. k_funm_combine exactly, at 8, 9, 16, 17 and 1024 steps (trips of 8 and a tail);
5. cgx_apply_function against eigh at n = 4100;
6. one projection + subtraction pass of cgx_eigenpairs exactly, at 16, 17 and 32 tiles and at 1, 31, 32, 33, 1023 and 1024 slots
   (the projection's grid of tiles x 32 chunks, hp[tile * 1040 + slot], the LDS array h[1040]);
7. the eigs basis: orthogonality, the Lanczos relation, the prefix property at 1024 and 300 steps;
8. cgx_eigenpairs: values, vectors, residuals, estimates.

n = 4096, 4100 and 7937 use the symmetric hash matrix, the references are lanczos_reference.lanczos_longdouble and numpy.linalg.eigh
of the dense matrix.  n = 8200 and 16400 use generate_lap2d_matrix (2.2 GB on the device at 16400, nothing is uploaded) and
lanczos_reference.Lap2dOperator on the host.  Every comparison with a high-precision reference is under
lanczos_reference.tolerance(d_cpu, n); the checking functions of the three modules run unchanged; every reference is computed here,
once per session (_CACHE), and none is hard-coded.  Each case prints n, tiles, g1 and, from the checking functions, d_cpu, d_dev and
the bar.

Left out:
- more than 1024 K1m partials at width 1 (a second trip of fold_pap there) and more than 256 tile partials (its second slot for
  the step kernels' own partials) both need n > 65536, a 34 GB matrix; the same trip of the same function runs at width 16, n = 8200;
- the 2^32-byte offset into the basis of cgx_apply_function needs 16 vectors x 1024 steps at n = 32768 (a 4 GB basis).
"""
import time

import numpy as np
import pytest

import eigs_reference as eref
import lanczos_reference as lref
import test_gpu_eigs as te
import test_gpu_funm as tf
import test_gpu_lanczos as tl

pytestmark = pytest.mark.gpu

NORM_LAP2D = 8.0     # ||generate_lap2d_matrix|| <= its largest absolute row sum, 4 + 4
SLQ_STEPS = 24       # the steps of the lap2d n = 16400 runs of tests 1 and 3
_CACHE = {}


def _width(nvec):
    return next(w for w in (1, 2, 4, 8, 16) if w >= nvec)          # multi_width (csrc/cgx_kernels.h)


def _grids(n, nvec):
    """(tiles, g1): the 256-row tiles and K1m's workgroups at the kernel width of nvec (MultiShape in csrc/cgx_device.h: 8 waves
    of 8, 4 or 1 rows)."""
    rows = {1: 64, 2: 64, 4: 64, 8: 32, 16: 8}[_width(nvec)]
    return -(-n // 256), -(-n // rows)


def _shape_line(n, nvec):
    tiles, g1 = _grids(n, nvec)
    slots = sorted({(f % 1024) // 256 for f in range(g1)})
    return "n=%d tiles=%d (fold of h: %d trips of 16, tail %d) nvec=%d width=%d g1=%d (fold_pap: %d trips, slots %s)" % (
        n, tiles, tiles // 16, tiles % 16, nvec, _width(nvec), g1, -(-g1 // 1024), slots)


def _timed(key, make):
    """_CACHE[key], made once per session; the time it took to make is kept for the log."""
    if key not in _CACHE:
        t0 = time.perf_counter()
        _CACHE[key] = make()
        print("reference %s: made in %.1f s" % (key, time.perf_counter() - t0))
    return _CACHE[key]


# ---- the matrices and their references, once per session ---------------------------------------------------------------------------
def _hash_matrix(oracle, n):
    """The symmetric hash matrix of the three modules and the 16 start vectors they use at this n."""
    def make():
        A = oracle.hash_rows(n, 0, n, tl.SEED, True, tl._diag(n))
        V0 = np.random.default_rng(1000 + n).standard_normal((16, n))
        tl._frozen(A, V0)
        return A, V0
    return _timed(("hash", n), make)


def _hash_eigh(oracle, n):
    """(A, lam, Q, V0); also placed where test_gpu_funm._hash_case looks for it, so that its checks use this decomposition."""
    def make():
        A, V0 = _hash_matrix(oracle, n)
        lam, Q = np.linalg.eigh(A)
        tl._frozen(lam, Q)
        tf._CACHE[("hash", n)] = (A, lam, Q, V0)
        return A, lam, Q, V0
    return _timed(("eigh", n), make)


def _hash_reorth(oracle, n, steps):
    """The float64 restatement of the eigs recurrence from the library's start vector; a shorter run is its leading part."""
    def make():
        run = eref.lanczos_reorth_f64(_hash_matrix(oracle, n)[0], te._start(n), steps)
        tl._frozen(run[0], run[1], run[3])
        return run
    return _timed(("reorth", n, steps), make)


def _lap2d(oracle, n):
    def make():
        V0 = np.random.default_rng(1000 + n).standard_normal((16, n))
        V0.setflags(write=False)
        return lref.Lap2dOperator(oracle, n), V0
    return _timed(("lap2d", n), make)


def _coefficient_refs(oracle, kind, n, steps):
    """Per start vector the longdouble recurrence and the float64 restatement of `steps` steps: (a_ref, b_ref, a_cpu, b_cpu, m_cpu)."""
    def make():
        A, V0 = _hash_matrix(oracle, n) if kind == "hash" else _lap2d(oracle, n)
        Al = A if lref.is_operator(A) else A.astype(np.longdouble)
        hi = [lref.lanczos_longdouble(Al, V0[j], steps) for j in range(16)]
        cpu = [lref.lanczos_f64(A, V0[j], steps) for j in range(16)]
        return tl._frozen(np.array([h[0] for h in hi]), np.array([h[1] for h in hi]), np.array([c[0] for c in cpu]),
                          np.array([c[1] for c in cpu]), np.array([c[2] for c in cpu]))
    return _timed(("coefficients", kind, n, steps), make)


def _solver(gpu_pkg, kind, n, **kw):
    if kind == "hash":
        return tl._hash_solver(gpu_pkg, n, **kw)
    s = gpu_pkg.CGSolver(gemv_variant=-1, **kw)
    s.generate_lap2d_matrix(n)
    return s


# ---- 1. cgx_lanczos ----------------------------------------------------------------------------------------------------------------
LANCZOS_CASES = {("hash", 4100): (12, (1, 2, 5, 8, 9, 16)), ("lap2d", 8200): (12, (8, 16)), ("lap2d", 16400): (SLQ_STEPS, (1, 3, 8, 16))}


def _lanczos_runs(gpu_pkg, oracle, kind, n):
    """What cgx_lanczos returns for the first nvec start vectors (every nvec of the case, and 8 and 16 for the width rule) and for
    the same vectors in reversed order, from one context."""
    if ("lanczos", kind, n) not in _CACHE:
        steps, nvecs = LANCZOS_CASES[(kind, n)]
        V0 = (_hash_matrix(oracle, n) if kind == "hash" else _lap2d(oracle, n))[1]
        got, rev = {}, {}
        with _solver(gpu_pkg, kind, n) as s:
            for nvec in sorted(set(nvecs) | {8, 16}):
                got[nvec] = s.lanczos(V0[:nvec], steps)
                rev[nvec] = s.lanczos(V0[:nvec][::-1], steps)
        _CACHE[("lanczos", kind, n)] = (got, rev)
    return _CACHE[("lanczos", kind, n)]


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


@pytest.mark.parametrize("kind,n,nvec", [(k, n, nvec) for (k, n), (_, nvecs) in LANCZOS_CASES.items() for nvec in nvecs])
def test_lanczos_coefficients(gpu_pkg, oracle, kind, n, nvec):
    steps = LANCZOS_CASES[(kind, n)][0]
    a_ref, b_ref, a_cpu, b_cpu, m_cpu = _coefficient_refs(oracle, kind, n, steps)
    got, rev = _lanczos_runs(gpu_pkg, oracle, kind, n)
    alpha, beta, done = got[nvec]
    print(kind, _shape_line(n, nvec))
    assert list(m_cpu[:nvec]) == [steps] * nvec, m_cpu            # the precondition, on the restatement: no column breaks down
    assert list(done) == [steps] * nvec, done
    tl._check_coefficients(n, nvec, steps, alpha, beta, done, a_ref, b_ref, a_cpu, b_cpu)
    # include/cgx.h, cgx_lanczos: a column depends on the kernel width of nvec only, and not on its position in the block
    wider = {5: 8, 9: 16}.get(nvec)
    if wider:
        aw, bw, donew = got[wider]
        assert np.array_equal(done, donew[:nvec])
        for name, x, y in (("alpha", alpha, aw), ("beta", beta, bw)):
            assert np.array_equal(_bits(x), _bits(y[:nvec])), (name, nvec, wider, float(np.abs(x - y[:nvec]).max()))
    ar, br, doner = rev[nvec]
    assert np.array_equal(done[::-1], doner)
    for name, x, y in (("alpha", alpha, ar), ("beta", beta, br)):
        assert np.array_equal(_bits(x[::-1]), _bits(y)), (name, nvec, "reversed", float(np.abs(x[::-1] - y).max()))


# ---- 2. breakdown beside running columns -------------------------------------------------------------------------------------------
def test_breakdown_and_freezing_at_17_tiles(gpu_pkg):
    print(_shape_line(4100, 4))
    tl._breakdown_and_freezing(gpu_pkg, 4, 4100)


# ---- 3. cgx_trace_slq --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nvec", LANCZOS_CASES[("lap2d", 16400)][1])
def test_slq_is_the_quadrature_of_the_recurrence(gpu_pkg, oracle, nvec):
    """per_probe[j] of logdet(Z = the start vectors of test 1) against lanczos_reference.quadrature of the device's own alpha and beta
    for the same vectors at the same kernel width: the estimator is tied to the recurrence, whose coefficients test 1 ties to the
    longdouble reference, with numpy.linalg.eigh of the Jacobi matrix as the second implementation of the rule.  The bar is the
    rule's floor, relative.  cgx_trace_slq runs its probes in batches of 8: 16 vectors are two runs at width 8, so columns 0 .. 7
    are compared with test 1's run of 8 and columns 8 .. 15 with a cgx_lanczos call on those 8 vectors."""
    n, steps = 16400, SLQ_STEPS
    V0 = _lap2d(oracle, n)[1]
    got, _ = _lanczos_runs(gpu_pkg, oracle, "lap2d", n)
    with _solver(gpu_pkg, "lap2d", n) as s:
        out = s.logdet(steps=steps, Z=V0[:nvec])
        tail = s.lanczos(V0[8:16], steps) if nvec > 8 else None
    print("lap2d", _shape_line(n, min(nvec, 8)))
    assert out["per_probe"].shape == (nvec,)
    for j in range(nvec):
        alpha, beta, done = (got[min(nvec, 8)] if j < 8 else tail)
        k = j if j < 8 else j - 8
        assert done[k] == steps
        want = lref.quadrature(alpha[k], beta[k], steps, float(V0[j] @ V0[j]), np.log)
        d_dev = abs(out["per_probe"][j] - want) / abs(want)
        print("slq n=%d nvec=%d probe %d: per_probe %.17g quadrature %.17g d_dev=%.3e bar=%.3e" % (
            n, nvec, j, out["per_probe"][j], want, d_dev, lref.tolerance(0.0, n)))
        assert d_dev <= lref.tolerance(0.0, n), (nvec, j, out["per_probe"][j], want)
    assert abs(out["estimate"] - np.mean(out["per_probe"])) <= 1e-14 * abs(out["estimate"])


# ---- 4. the funm combine kernel, exactly -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lda_pad", [-1, 0])                      # the default pitch; roundup(n, 16), no pad columns
def test_funm_combine_is_exact(gpu_pkg, lda_pad):
    """Trips of 8 steps and a tail: 8 (one trip), 9 (a trip and one), 16, 17, 1024 (CGX_MAX_LANCZOS_STEPS: 128 trips); every
    column's own m[j] in 1 .. steps, non-finite values behind it."""
    n = 4100
    rng = np.random.default_rng(10 * n + lda_pad + 1)
    print(_shape_line(n, 1))
    with gpu_pkg.CGSolver(gemv_variant=-1, lda_pad=lda_pad) as s:          # the kernel reads no matrix: any n x n one will do
        s.generate_lap2d_matrix(n)
        for steps, nvec in ((8, 16), (9, 3), (16, 1), (17, 8), (1024, 1), (1024, 3)):
            tf._combine_case(s, rng, n, nvec, steps)


# ---- 5. cgx_apply_function ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nvec", [2, 16])
def test_apply_function_against_eigh(gpu_pkg, oracle, nvec):
    n = 4100
    _hash_eigh(oracle, n)
    print("hash", _shape_line(n, nvec))
    tf._hash_matrix_against_eigh(gpu_pkg, oracle, n, nvec, 24)


# ---- 6. the eigs pass, exactly -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,lda_pad", [(4096, -1), (4100, -1), (4100, 0), (7937, -1)])
def test_eigs_pass_is_exact(gpu_pkg, n, lda_pad):
    """test_gpu_eigs.test_pass_is_exact's body.  Bit-exactness in any sum order needs |h| <= 64 n and |w_out| <= 8 + 8 nslots 64 n
    below 2^53: 4.2e9 at n = 7937 with 1024 slots (the body asserts < 2^50 on the values themselves)."""
    c, most = gpu_pkg.cgx.EIGS_SLOT_CHUNK, gpu_pkg.cgx.MAX_LANCZOS_STEPS
    assert (c, most) == (32, 1024)
    tiles = _grids(n, 1)[0]
    print("n=%d lda_pad=%d tiles=%d (fold of h: %d trips of 16, tail %d); projection grid up to %d x %d" % (
        n, lda_pad, tiles, tiles // 16, tiles % 16, tiles, most // c))
    with gpu_pkg.CGSolver(gemv_variant=-1, lda_pad=lda_pad) as s:
        s.generate_lap2d_matrix(n)
        te._pass_is_exact(s, n, lda_pad, (1, c - 1, c, c + 1, most - 1, most, 2))   # the last one reuses the larger block


# ---- 7. the eigs basis -------------------------------------------------------------------------------------------------------------
def _hash_basis(gpu_pkg, oracle, n):
    if ("basis", n) not in _CACHE:
        with tl._hash_solver(gpu_pkg, n) as s:
            _CACHE[("basis", n)] = {steps: s._probe_eigs_basis(te._start(n), steps) for steps in (1024, 300)}
    return _CACHE[("basis", n)]


def _check_basis(tag, n, A, norm, run, steps, dev):
    Q, alpha, beta, m = dev
    assert m == steps and run[2] >= steps, (m, run[2])
    o_cpu, r_cpu = te._basis_figures(A, norm, run[0], run[1], steps, run[3])
    o_dev, r_dev = te._basis_figures(A, norm, alpha, beta, m, Q)
    print("%s steps=%d: max |Q Q^T - I| d_cpu=%.3e d_dev=%.3e bar=%.3e; relation d_cpu=%.3e d_dev=%.3e bar=%.3e" % (
        tag, steps, o_cpu, o_dev, lref.tolerance(o_cpu, n), r_cpu, r_dev, lref.tolerance(r_cpu, n)))
    assert o_dev <= lref.tolerance(o_cpu, n), (o_cpu, o_dev)
    assert r_dev <= lref.tolerance(r_cpu, n), (r_cpu, r_dev)


@pytest.mark.parametrize("steps", [1024, 300])
def test_eigs_basis_on_the_hash_matrix(gpu_pkg, oracle, steps):
    n = 4100
    A, lam, _, _ = _hash_eigh(oracle, n)
    run = _hash_reorth(oracle, n, 1024)
    print("hash", _shape_line(n, 1))
    _check_basis("hash n=%d" % n, n, A, float(np.max(np.abs(lam))), run, steps, _hash_basis(gpu_pkg, oracle, n)[steps])


def test_eigs_basis_prefix_property(gpu_pkg, oracle):
    """alpha, beta and q_0 .. q_300 of the 300-step run inside the 1024-step run, bit for bit: no grid, tile or sum order of
    csrc/cgx_eigs.hip depends on the steps of the call."""
    runs = _hash_basis(gpu_pkg, oracle, 4100)
    (Q, alpha, beta, m), (Q3, a3, b3, m3) = runs[1024], runs[300]
    assert (m, m3) == (1024, 300)
    assert np.array_equal(_bits(a3), _bits(alpha[:300])) and np.array_equal(_bits(b3), _bits(beta[:300]))
    assert np.array_equal(_bits(Q3[:301]), _bits(Q[:301]))


def _lap2d_eigs_refs(oracle, n, steps):
    """From the library's start vector: the float64 restatement of the eigs recurrence and the longdouble recurrence, `steps` steps
    each (a shorter run is the leading part of either)."""
    def make():
        op = _lap2d(oracle, n)[0]
        run = eref.lanczos_reorth_f64(op, te._start(n), steps)
        a_ld, b_ld = lref.lanczos_longdouble(op, te._start(n), steps)
        tl._frozen(run[0], run[1], run[3], a_ld, b_ld)
        return run, a_ld, b_ld
    return _timed(("lap2d eigs", n, steps), make)


def test_eigs_basis_on_lap2d(gpu_pkg, oracle):
    n, steps = 16400, 40
    op = _lap2d(oracle, n)[0]
    run, a_ld, b_ld = _lap2d_eigs_refs(oracle, n, 64)
    with _solver(gpu_pkg, "lap2d", n) as s:
        dev = s._probe_eigs_basis(te._start(n), steps)
    print("lap2d", _shape_line(n, 1))
    _check_basis("lap2d n=%d" % n, n, op, NORM_LAP2D, run, steps, dev)
    Q, alpha, beta, m = dev
    tl._check_coefficients(n, 1, steps, alpha[None, :], beta[None, :], [m], a_ld[None, :steps], b_ld[None, :steps],
                           run[0][None, :steps], run[1][None, :steps])


# ---- 8. cgx_eigenpairs -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["largest", "smallest"])
def test_eigenpairs_on_the_hash_matrix(gpu_pkg, oracle, which):
    n = 4100
    A, lam, Qe, _ = _hash_eigh(oracle, n)
    print("hash", _shape_line(n, 8))
    te._hash_matrix_against_eigh(gpu_pkg, n, 8, 300, which, (A, lam, Qe, _hash_reorth(oracle, n, 1024)))


def test_eigenpairs_do_not_depend_on_how_many_are_asked_for(gpu_pkg, oracle):
    n, steps = 4100, 300
    outs = {}
    with tl._hash_solver(gpu_pkg, n) as s:
        for nev in (1, 3, 8, 16):
            outs[nev] = s.eigenpairs(nev, "largest", steps)
    for nev in (1, 3, 8, 16):
        vals, X, info = outs[nev]
        print("hash", _shape_line(n, nev))
        assert info["steps_done"] == steps and info["nfound"] == nev
        assert np.array_equal(_bits(vals), _bits(outs[16][0][:nev])) and np.array_equal(_bits(X), _bits(outs[16][1][:nev])), nev


def test_eigenpairs_on_lap2d(gpu_pkg, oracle):
    """Values and residuals only: the extreme eigenvalues of generate_lap2d_matrix are nearly multiple, so a wanted eigenvector is fixed only up to a rotation within its cluster and the
    vectors of two correct runs need not agree; the residual, checked against a host recomputation from the device's own pair,
    is what says that each returned vector belongs to its value.  The values are compared with the Ritz values of the longdouble
    recurrence's Jacobi matrix: after 64 steps they have not converged to eigenvalues, and device, restatement and reference share
    the truncation."""
    n, steps, nev = 16400, 64, 4
    op = _lap2d(oracle, n)[0]
    run, a_ld, b_ld = _lap2d_eigs_refs(oracle, n, steps)
    assert run[2] == steps
    theta = np.linalg.eigvalsh(lref.jacobi_matrix(a_ld, b_ld, steps))[::-1][:nev]
    cpu = eref.eigenpairs_f64(op, None, eref.LARGEST, nev, steps, run=run)
    with _solver(gpu_pkg, "lap2d", n) as s:
        vals, X, info = s.eigenpairs(nev, "largest", steps)
    print("lap2d", _shape_line(n, nev))
    assert info["steps_done"] == steps and info["nfound"] == nev
    d_cpu, d_dev = float(np.max(np.abs(cpu[0] - theta))) / NORM_LAP2D, float(np.max(np.abs(vals - theta))) / NORM_LAP2D
    print("lap2d n=%d steps=%d: values d_cpu=%.3e d_dev=%.3e bar=%.3e" % (n, steps, d_cpu, d_dev, lref.tolerance(d_cpu, n)))
    assert d_dev <= lref.tolerance(d_cpu, n), (vals, theta)
    assert np.all(np.diff(vals) < 0.0)
    for j in range(nev):
        host = float(np.linalg.norm(op @ X[j] - vals[j] * X[j]))
        print("lap2d n=%d pair %d: value %.17g residual %.6e host %.6e (bar %.3e)" % (
            n, j, vals[j], info["residual"][j], host, lref.tolerance(0.0, n) * NORM_LAP2D))
        assert abs(info["residual"][j] - host) <= lref.tolerance(0.0, n) * NORM_LAP2D, (j, info["residual"][j], host)
