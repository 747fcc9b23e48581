"""The pivoted-Cholesky kernels (csrc/cgx_lowrank.hip, csrc/cgx_multi_pc.hip, csrc/cgx_lanczos_pc.hip) past 16 row tiles and at
every kernel width.

The other modules stop at n = 1101, G = ceil(n / 256) = 5 tiles, and at the widths 1, 3, 8, 16.  The fold of t = L^T r over the tiles
runs 16 tiles at a time with a scalar tail (lr_fold_tiles in csrc/cgx_lowrank_cols.h: one function, called by k_lr_apply and by the
one apply body lr_apply_cols that k_multi_lr_apply and k_lpc_lr_apply wrap), the apply kernels are templates of the width 1, 2, 4,
8 or 16 with dead columns in a partly filled one, and a Lanczos column that freezes under this preconditioner goes through
k_lpc_lr_step / k_lpc_lr_apply, not through the Jacobi kernel the breakdown test runs.  Here:

  n = 4096   G = 16   one full trip of the fold, no tail, no ragged tile
  n = 4100   G = 17   one trip and a tail of one tile, whose last tile has 4 rows
  n = 7937   G = 32   two trips, no tail, a last tile of 1 row

1. the factor and the apply of the single path against the longdouble restatements (test_gpu_pivchol's own checks);
2. a converged single solve against numpy PCG in fp64 and longdouble;
3. z = M^-1 r of the multi kernels, every k in 1 .. 16, against the single path's, bit for bit;
4. cgx_solve_multi_pc: fixed iterations against longdouble PCG, converged columns, column 0 against the single solve;
5. cgx_lanczos_pc: the coefficients against the longdouble recurrence, and the width rule of include/cgx.h;
6. a column that freezes under the pivoted-Cholesky factor beside running ones.

Every factor is the device's own (L and delta through the probe), every bar is the one the same quantity meets in
test_gpu_pivchol.py, test_gpu_multi_pc.py and test_gpu_lanczos_pc.py, whose checking functions run here unchanged.  Every reference
number is computed here; none is hard-coded."""
import numpy as np
import pytest

import lanczos_pc_reference as lpref
import lanczos_reference as lref
import pivchol_reference as ref
import test_gpu_lanczos_pc as lp
import test_gpu_multi_pc as mp
import test_gpu_pivchol as pv

pytestmark = pytest.mark.gpu

KS = (2, 5, 9, 16)   # width 2; widths 8 and 16 partly filled; width 16 full
STEPS = lp.STEPS
_CACHE = {}


def _pitch(pad):
    return {} if pad is None else {"lda_pad": pad}


# ---- 1. the factor and the apply of the single path --------------------------------------------------------------------------------
@pytest.mark.parametrize("n,rank,pad", [(4096, 64, None), (4100, 100, None), (4100, 100, 0), (4100, 5, None), (7937, 16, None)])
def test_factor_and_apply_single_path(gpu_pkg, n, rank, pad):
    """pad 0: the pitch is roundup(n, 16), the columns of L touch but for that."""
    f = pv._device_factor(gpu_pkg, n, rank, **_pitch(pad))
    pv._check_factor(f, n, rank)
    pv._check_apply(f, n, rank)
    for name, z in f["z"].items():
        assert np.all(np.isfinite(z)) and np.any(z != 0.0), name
    if pad is not None:                                       # the pitch changes no bit (test_gpu_row_pitch.py's rule)
        f16 = pv._device_factor(gpu_pkg, n, rank)
        assert np.array_equal(f["piv"], f16["piv"]) and np.array_equal(f["L"], f16["L"]) and f["delta"] == f16["delta"]
        for name in f["z"]:
            assert np.array_equal(f["z"][name], f16["z"][name]), name


# ---- 2. the single solve -----------------------------------------------------------------------------------------------------------
def _single_solve(gpu_pkg, n, rank):
    """(x, result, L, delta) of a converged single solve, once per session."""
    if ("single", n, rank) not in _CACHE:
        with pv._solver(gpu_pkg, n) as s:
            s.set_preconditioner("pivchol", rank=rank)
            x = np.zeros(n)
            res = s.solve(x)
            _, L, delta = s._probe_precond_lowrank()
        _CACHE[("single", n, rank)] = (x, res, L, delta)
    return _CACHE[("single", n, rank)]


@pytest.mark.parametrize("rank", [100, 128])   # (ranks 16 and 64 do not give a clear stop at this n: pv._references refuses them)
def test_solve_single_path(gpu_pkg, rank):
    n = 4100
    x, res, L, delta = _single_solve(gpu_pkg, n, rank)
    k = pv._check_solve(x, res, n, L, delta)
    print("n=%d rank=%d: %d iterations" % (n, rank, k))


# ---- 3. the multi apply ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,rank,pad", [(4100, 100, None), (4100, 100, 0), (4100, 5, None), (7937, 16, None)])
def test_multi_apply_has_the_single_paths_bits(gpu_pkg, n, rank, pad):
    """test_gpu_multi_pc.test_apply_matches_the_single_path at G = 17 and 32, every k: with test 1 this ties every width of
    k_multi_lr_update<true> and k_multi_lr_apply<W> to the longdouble Woodbury apply."""
    _, _, B16, _ = mp._kernel_problem(n)
    R = np.array(B16)
    R[5] = 0.0
    R[5, 7] = 1.0
    with mp._kernel_solver(gpu_pkg, n, rank, **_pitch(pad)) as s:
        s.set_max_iter(1)
        s.tolerance(0.0)
        s.solve_multi_pc(R[:3])                               # the multi call makes the factor ...
        single = np.array([s._probe_precond_apply(R[j]) for j in range(16)])   # ... the single path's kernels use it
        Z = {k: s._probe_multi_pc_apply(R[:k]) for k in range(1, 17)}
    assert np.all(np.isfinite(single)) and all(np.linalg.norm(single[j]) > 0 for j in range(16))
    for k in range(1, 17):
        assert np.all(np.isfinite(Z[k])) and np.linalg.norm(Z[k]) > 0, k
        same = np.all(Z[k].view(np.uint64) == single[:k].view(np.uint64), axis=1)
        print("n=%d rank=%d pad=%s k=%d: max |Z - single| = %.3e" % (n, rank, pad, k, float(np.abs(Z[k] - single[:k]).max())))
        assert np.all(same), (k, np.flatnonzero(~same).tolist(), float(np.abs(Z[k] - single[:k]).max()))


# ---- 4. cgx_solve_multi_pc ---------------------------------------------------------------------------------------------------------
def test_solve_multi_pc_fixed_iterations(gpu_pkg):
    n, rank, iters = 4100, 64, 12
    A, b, B, X0 = mp._kernel_problem(n)
    out = {}
    with mp._kernel_solver(gpu_pkg, n, rank) as s:
        s.set_max_iter(iters)
        s.tolerance(0.0)
        for k in KS:
            out[k] = s.solve_multi_pc(B[:k], X0[:k])
        _, L, delta = s._probe_precond_lowrank()
    r64, rld = mp._references(("fix", n, rank), A, B, X0, (ref.Woodbury(L, delta, np.float64).apply, ref.Woodbury(L, delta, ref.LD).apply),
                              0.0, iters)
    for k, (X, res) in out.items():
        for j in range(k):
            assert res[j]["iterations"] == iters == rld[j]["iterations"] and res[j]["converged"] == 0, (k, j, res[j])
            mp._check_x(X[j], r64[j], rld[j], "n=%d rank=%d k=%d column %d" % (n, rank, k, j))
            assert res[j]["gemv_bytes"] == 8.0 * (n * n + 2.0 * k * n)

    # converged columns at rank 100; column 0 is the single solve's problem (b, zero guess)
    rank = 100
    tol = 1e-6 * float(np.linalg.norm(b))
    xs, ress, Ls, deltas = _single_solve(gpu_pkg, n, rank)
    conv = {}
    with mp._kernel_solver(gpu_pkg, n, rank) as s:
        for k in (2, 5):
            conv[k] = s.solve_multi_pc(B[:k])
        _, L, delta = s._probe_precond_lowrank()
    assert np.array_equal(L, Ls) and delta == deltas          # one factor: one longdouble reference for both paths
    s64, sld = pv._references(n, L, delta, tol)
    mp._check_x(xs, s64, sld, "rank %d, the single solve" % rank)
    for k, (X, res) in conv.items():
        for j in range(k):
            assert res[j]["converged"] == 1, (k, j, res[j])
            assert res[j]["rel_residual"] <= 10 * tol / float(np.linalg.norm(B[j])), (k, j, res[j])
        mp._check_x(X[0], s64, sld, "rank %d k=%d column 0" % (rank, k))
        assert res[0]["iterations"] == sld["iterations"] == ress["iterations"], (k, res[0], sld["iterations"], ress["iterations"])


# ---- 5. cgx_lanczos_pc -------------------------------------------------------------------------------------------------------------
def _lanczos_runs(gpu_pkg, n, rank):
    """What cgx_lanczos_pc returns for the first nvec start vectors, nvec in KS and 8, and the references, once per session."""
    if ("lanczos", n, rank) not in _CACHE:
        A, V0 = lp._kernel(n), lp._start_vectors(n)
        with lp._kernel_solver(gpu_pkg, n, rank) as s:
            got = {nvec: s.lanczos_pc(V0[:nvec], STEPS) for nvec in KS + (8,)}
            _, L, delta = s._probe_precond_lowrank()          # the device's own factor
        refs = lp._references(("pc", n, rank), A, V0, lpref.lowrank_apply(L, delta), lpref.lowrank_apply(L, delta, lpref.LD))
        _CACHE[("lanczos", n, rank)] = (got, refs)
    return _CACHE[("lanczos", n, rank)]


@pytest.mark.parametrize("nvec", KS)
@pytest.mark.parametrize("n,rank", [(4100, 64), (4100, 5)])
def test_lanczos_pc_coefficients(gpu_pkg, n, rank, nvec):
    got, refs = _lanczos_runs(gpu_pkg, n, rank)
    lp._check_coefficients("pivchol n=%d rank=%d" % (n, rank), n, got[nvec], refs, nvec)
    # include/cgx.h, cgx_lanczos_pc: a column depends on the kernel width of nvec only
    wider = {5: 8, 9: 16}.get(nvec)
    if wider:
        (a, b, done, e2), (aw, bw, donew, e2w) = got[nvec], got[wider]
        assert np.array_equal(done, donew[:nvec]), (nvec, wider)
        for name, x, y in (("alpha", a, aw), ("beta", b, bw), ("eta2", e2, e2w)):
            assert np.array_equal(x.view(np.uint64), y[:nvec].view(np.uint64)), (name, nvec, wider, float(np.abs(x - y[:nvec]).max()))


# ---- 6. a frozen column under the pivoted-Cholesky factor --------------------------------------------------------------------------
@pytest.mark.parametrize("n,rank", [(4100, 5), (1101, 16)])
def test_lanczos_pc_frozen_column_under_pivchol(gpu_pkg, n, rank):
    """Column 1 of four starts from w = M u, u the eigenvector of the largest theta of A u = theta M u: u_0 = M^-1 w = u, A u_0 =
    theta w, so alpha_0 = theta and w_1 is rounding only -- the column freezes at m = 1 between three that run (k_lpc_lr_step's
    step_head, then s_live in both kernels).  The test asserts on the float64 restatement, never on the device's output, that the
    start does freeze with a margin of 16 below the threshold; rank 64 leaves a margin of 1.5 and is not used.  theta is scipy's
    eigenvector put through the Rayleigh quotient u.Au / u.Mu in longdouble (an error of the vector enters squared), so that the
    reference's own error stays below n 2^-52."""
    import scipy.linalg
    A, Z = lp._kernel(n), lp._start_vectors(n)[:4]
    with lp._kernel_solver(gpu_pkg, n, rank) as s:
        alpha3, beta3, done3, eta3 = s.lanczos_pc(np.array([Z[0], Z[3], Z[1], Z[2]]), STEPS)   # the same width, no frozen column
        _, L, delta = s._probe_precond_lowrank()
        M = L @ L.T + delta * np.eye(n)
        theta64, U = scipy.linalg.eigh(A, M, subset_by_index=[n - 1, n - 1])
        u = U[:, 0]
        w = M @ u
        V = np.array([Z[0], w, Z[1], Z[2]])
        alpha2, beta2, done2, eta2 = s.lanczos_pc(V, STEPS)
    ul, Ll, Al = u.astype(lpref.LD), L.astype(lpref.LD), lp._longdouble(A)
    theta = float((ul @ (Al @ ul)) / (ul @ (Ll @ (Ll.T @ ul) + lpref.LD(delta) * ul)))
    ap64 = lpref.lowrank_apply(L, delta)
    a_cpu, b_cpu, m_cpu, _ = lpref.lanczos_pc_f64(A, ap64, w, STEPS)
    print("n=%d rank=%d: theta %.17g (eigh %.17g); float64 restatement m=%d, beta_0/|alpha_0| = %.3e (threshold 2^-36 / 16 = %.3e)" % (
        n, rank, theta, float(theta64[0]), m_cpu, b_cpu[0] / abs(a_cpu[0]), lref.BREAK / 16))
    assert m_cpu == 1 and b_cpu[0] / abs(a_cpu[0]) <= lref.BREAK / 16   # the precondition: the start freezes, and clearly
    assert list(done3) == [STEPS] * 4, done3
    assert list(done2) == [STEPS, 1, STEPS, STEPS], done2
    assert np.all(alpha2[1, 1:] == 0) and np.all(beta2[1, 1:] == 0)
    bar = lref.tolerance(abs(a_cpu[0] - theta) / theta, n) * theta
    print("eigenvector start: alpha_0 - theta = %.3e (float64 %.3e, bar %.3e), beta_0 = %.3e" % (
        alpha2[1, 0] - theta, a_cpu[0] - theta, bar, beta2[1, 0]))
    assert abs(alpha2[1, 0] - theta) <= bar
    assert beta2[1, 0] <= lref.BREAK * abs(alpha2[1, 0])
    for col in (0, 2, 3):                                     # the running columns: the bits of the call without the frozen one
        assert np.array_equal(alpha2[col].view(np.uint64), alpha3[col].view(np.uint64)), col
        assert np.array_equal(beta2[col].view(np.uint64), beta3[col].view(np.uint64)), col
        assert eta2[col] == eta3[col], col
    run = [0, 2, 3]                                           # ... and the longdouble recurrence of their start vectors
    refs = lp._references(("pc frozen", n, rank), A, Z[:3], ap64, lpref.lowrank_apply(L, delta, lpref.LD))
    lp._check_coefficients("pivchol n=%d rank=%d beside a frozen column" % (n, rank), n, (alpha2[run], beta2[run], done2[run], eta2[run]), refs, 3)
