"""cgx_eigenpairs / cgx_probe_eigs_basis / cgx_probe_eigs_orthogonalise (csrc/cgx_eigs.hip) on the MI355X.

- one projection + subtraction pass alone, exactly, on integer slots with non-finite values wherever the kernels must not read;
- the basis: orthogonality, the Lanczos relation, the bitwise prefix property;
- values, vectors, residuals and estimates on the symmetric hash matrix and on a kernel matrix against numpy.linalg.eigh;
- no ghosts where the plain recurrence has them; invariant subspaces on A = H D H; the tol-driven form;
- widths and edges, determinism, no interference with the other paths, refusals, the fault walk, the command line.

The tolerance rule is that of tests/test_gpu_lanczos.py: wherever a device result is compared with a reference, the test computes
d_cpu, the deviation of the float64 numpy restatement of the same recurrence (tests/eigs_reference.py) from that reference, and
allows the device 16 max(d_cpu, n 2^-52), relative to the norm of the reference (lanczos_reference.tolerance); eigenvectors are
compared after aligning the sign.  A truncated run passes under the same rule because device and restatement share the truncation.

Past 16 row tiles and at 1024 slots (n = 4096 .. 16400): tests/test_gpu_lanczos_tiles.py.
"""
import os
import re
import subprocess

import numpy as np
import pytest

import eigs_reference as eref
import lanczos_reference as ref
import pivchol_reference as pcref

pytestmark = pytest.mark.gpu

SEED = 0x3D1F                                          # the hash matrix of tests/test_gpu_funm.py
ERR_BAD_ARG, ERR_HIP, ERR_UNSUPPORTED = 1, 3, 7        # cgx_status (include/cgx.h)
_CACHE = {}


def _diag(n):
    return 1.03 * 2.0 * np.sqrt(n / 3.0)


def _hash_solver(pkg, n, **kw):
    s = pkg.CGSolver(gemv_variant=kw.pop("gemv_variant", -1), **kw)
    s.generate_lap2d_matrix(n)
    s.probe_fill_matrix_hash(SEED, symmetric=True, diag=_diag(n))
    return s


def _dense_solver(pkg, A, **kw):
    s = pkg.CGSolver(gemv_variant=-1, **kw)
    s.set_matrix_dense(A)
    return s


def _start(n):
    return ref.rademacher(1, 1, n)[0]                  # what v0 = NULL, seed = 1 means


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)


def _hash_case(oracle, n):
    """Made once per n and left unchanged: the matrix, its eigen-decomposition and the restatement's run of 300 (257) steps."""
    if ("hash", n) not in _CACHE:
        A = oracle.hash_rows_numpy(n, np.arange(n), SEED, True, _diag(n))
        lam, Q = np.linalg.eigh(A)
        run = eref.lanczos_reorth_f64(A, _start(n), min(n, 300))
        _frozen(A, lam, Q, run[0], run[1], run[3])
        _CACHE[("hash", n)] = (A, lam, Q, run)
    return _CACHE[("hash", n)]


def _kernel_case():
    if "kernel" not in _CACHE:
        K, _ = pcref.kernel_matrix(1024, 0.2, 1e-2)
        lam, Q = np.linalg.eigh(K)
        run = eref.lanczos_reorth_f64(K, _start(1024), 300)
        _frozen(lam, Q, run[0], run[1], run[3])
        _CACHE["kernel"] = (K, lam, Q, run)
    return _CACHE["kernel"]


def _cut(run, steps):
    """The restatement's run of fewer steps: the leading part of a longer one (the prefix property)."""
    return (run[0][:steps], run[1][:steps], min(run[2], steps), run[3][:steps + 1])


# ---- 1. the pass, exactly ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,lda_pad", [(1, -1), (255, -1), (257, -1), (1000, -1), (257, 0)])
def test_pass_is_exact(gpu_pkg, n, lda_pad):
    """Integer slots and w with |values| <= 8: every product and sum stays below 2^53, so any order gives the same bits.  On the
    host the rows behind nslots, the columns behind n and w's tail hold NaN / inf; on the device the probe fills the slots it uses,
    the slot behind them and w with NaN over the whole row pitch before it uploads the n columns (include/cgx.h)."""
    c = gpu_pkg.cgx.EIGS_SLOT_CHUNK
    with _dense_solver(gpu_pkg, 2.0 * np.eye(n), lda_pad=lda_pad) as s:
        _pass_is_exact(s, n, lda_pad, (1, 2, 37, c - 1, c, c + 1, 2))   # the last one reuses the larger block


def _pass_is_exact(s, n, lda_pad, slot_counts):
    """The pass on the context s (any n x n matrix: the pass does not read it) for every nslots of slot_counts.  Also run by
    tests/test_gpu_lanczos_tiles.py past 16 tiles and at 1024 slots."""
    rng = np.random.default_rng(10 * n + lda_pad + 1)
    poison = [np.nan, np.inf, -np.inf]
    for nslots in slot_counts:
        Q = np.full((nslots + 2, n + 3), np.nan)
        Q[:nslots, :n] = rng.integers(-8, 9, (nslots, n))
        for r in range(nslots + 2):
            Q[r, n:] = poison[r % 3]
        Q[nslots] = np.inf
        Q[nslots + 1] = -np.inf
        w = np.full(n + 2, np.nan)
        w[:n] = rng.integers(-8, 9, n)
        want_h = Q[:nslots, :n] @ w[:n]
        want_w = w[:n] - want_h @ Q[:nslots, :n]
        assert np.max(np.abs(want_w)) < 2.0 ** 50
        h, out = s._probe_eigs_orthogonalise(Q, w, nslots)
        assert np.array_equal(h, want_h), (n, nslots, np.argwhere(h != want_h)[:4])
        assert np.array_equal(out, want_w), (n, nslots, np.argwhere(out != want_w)[:4])


# ---- 2. the basis -----------------------------------------------------------------------------------------------------------------
def _basis_figures(A, norm, alpha, beta, m, Q):
    Qm = Q[:m]
    orth = float(np.max(np.abs(Qm @ Qm.T - np.eye(m))))
    R = A @ Qm.T - Qm.T @ ref.jacobi_matrix(alpha, beta, m)
    if beta[m - 1] > ref.BREAK * np.max(np.abs(alpha[:m])):       # not frozen in the last step: q_m is there
        R[:, m - 1] -= beta[m - 1] * Q[m]
    return orth, float(np.linalg.norm(R, 2)) / norm


@pytest.mark.parametrize("n,steps", [(257, 257), (1000, 120)])
def test_basis_is_orthogonal_and_a_lanczos_basis(gpu_pkg, oracle, n, steps):
    A, lam, _, run = _hash_case(oracle, n)
    norm = float(np.max(np.abs(lam)))
    with _hash_solver(gpu_pkg, n) as s:
        Q, alpha, beta, m = s._probe_eigs_basis(_start(n), steps)
        if n == 1000:
            Q60, a60, b60, m60 = s._probe_eigs_basis(_start(n), 60)
    assert m == steps
    o_cpu, r_cpu = _basis_figures(A, norm, run[0], run[1], steps, run[3])
    o_dev, r_dev = _basis_figures(A, norm, alpha, beta, m, Q)
    print("hash n=%d steps=%d: max |Q Q^T - I| cpu %.3e dev %.3e; relation cpu %.3e dev %.3e" % (n, steps, o_cpu, o_dev, r_cpu, r_dev))
    assert o_dev <= ref.tolerance(o_cpu, n), (o_cpu, o_dev)
    assert r_dev <= ref.tolerance(r_cpu, n), (r_cpu, r_dev)
    if n == 1000:                                                 # the prefix property, bit for bit
        assert m60 == 60
        assert np.array_equal(a60, alpha[:60]) and np.array_equal(b60, beta[:60]) and np.array_equal(Q60[:61], Q[:61])


# ---- 3. values and vectors --------------------------------------------------------------------------------------------------------
def _compare(tag, n, norm, got, cpu, lam_w, X_w, A):
    vals, X, info = got
    vals_c, X_c, info_c = cpu
    nev = len(vals)
    dv_cpu, dv_dev = float(np.max(np.abs(vals_c - lam_w))) / norm, float(np.max(np.abs(vals - lam_w))) / norm
    print("%s: values d_cpu=%.3e d_dev=%.3e tol=%.3e" % (tag, dv_cpu, dv_dev, ref.tolerance(dv_cpu, n)))
    assert dv_dev <= ref.tolerance(dv_cpu, n), (tag, dv_cpu, dv_dev)
    if X_w is not None:
        for j in range(nev):
            dx_cpu = float(np.linalg.norm(eref.align(X_c[j], X_w[j])[0] - X_w[j]))
            dx_dev = float(np.linalg.norm(eref.align(X[j], X_w[j])[0] - X_w[j]))
            print("%s: vector %d d_cpu=%.3e d_dev=%.3e tol=%.3e" % (tag, j, dx_cpu, dx_dev, ref.tolerance(dx_cpu, n)))
            assert dx_dev <= ref.tolerance(dx_cpu, n), (tag, j, dx_cpu, dx_dev)
    # the residual is a true one: against a host recomputation from the device's own pair, to the floor of the rule times ||A||
    for j in range(nev):
        host = float(np.linalg.norm(A @ X[j] - vals[j] * X[j]))
        assert abs(info["residual"][j] - host) <= ref.tolerance(0.0, n) * norm, (tag, j, info["residual"][j], host)
    print("%s: residuals / ||A|| dev %.3e cpu %.3e" % (tag, np.max(info["residual"]) / norm, np.max(info_c["residual"]) / norm))
    assert np.max(info["residual"]) / norm <= ref.tolerance(np.max(info_c["residual"]) / norm, n)


def _check_estimates(tag, n, norm, s, v0, steps, which, nev, info):
    """estimate_j = beta_(m-1) |last component of T's eigenvector| from the device's OWN alpha and beta (the probe runs the same
    recurrence, bit for bit), the eigenvectors by numpy.linalg.eigh: to the floor of the rule times ||A||."""
    _, alpha, beta, m = s._probe_eigs_basis(v0, steps)
    assert m == info["steps_done"]
    _, _, est, _, _ = eref.ritz(alpha, beta, m, which, nev)
    d = float(np.max(np.abs(info["estimate"][:len(est)] - est)))
    print("%s: estimates up to %.3e, against beta |s| of the device's T: %.3e" % (tag, np.max(info["estimate"]), d))
    assert d <= ref.tolerance(0.0, n) * norm, (tag, d)


@pytest.mark.parametrize("which", ["largest", "smallest"])
@pytest.mark.parametrize("steps", [300, 200])
def test_hash_matrix_against_eigh(gpu_pkg, oracle, steps, which):
    _hash_matrix_against_eigh(gpu_pkg, 1000, 8, steps, which, _hash_case(oracle, 1000))


def _hash_matrix_against_eigh(gpu_pkg, n, nev, steps, which, case):
    """case: (A, lam, Qe, run) as _hash_case makes it, run of at least `steps` steps.  (tests/test_gpu_lanczos_tiles.py: n = 4100.)"""
    A, lam, Qe, run = case
    norm = float(np.max(np.abs(lam)))
    w = eref.LARGEST if which == "largest" else eref.SMALLEST
    cpu = eref.eigenpairs_f64(A, None, w, nev, steps, run=_cut(run, steps))
    lam_w, X_w = eref.wanted(lam, Qe, w, nev)
    with _hash_solver(gpu_pkg, n) as s:
        got = s.eigenpairs(nev, which, steps)
        assert got[2]["steps_done"] == steps and got[2]["nfound"] == nev
        _check_estimates("hash %s %d" % (which, steps), n, norm, s, _start(n), steps, w, nev, got[2])
    _compare("hash n=%d %s steps=%d" % (n, which, steps), n, norm, got, cpu, lam_w, X_w, A)
    assert np.all(np.diff(got[0]) < 0.0) if which == "largest" else np.all(np.diff(got[0]) > 0.0)


def test_kernel_matrix_largest(gpu_pkg):
    n, nev = 1024, 8
    K, lam, Qe, run = _kernel_case()
    norm = float(lam[-1])
    lam_w, X_w = eref.wanted(lam, Qe, eref.LARGEST, nev)
    with _dense_solver(gpu_pkg, K) as s:
        got60 = s.eigenpairs(nev, "largest", 60)
        got300 = s.eigenpairs(nev, "largest", 300)
    assert got60[2]["steps_done"] == 60
    _compare("kernel n=1024 60 steps", n, norm, got60, eref.eigenpairs_f64(K, None, eref.LARGEST, nev, 60, run=_cut(run, 60)), lam_w, X_w, K)
    # 300 steps: the run freezes at an invariant subspace (the restatement at 188); the device's count may differ from that by
    # the tolerance of the beta test only
    print("kernel n=1024 300 steps: steps_done %d (restatement %d)" % (got300[2]["steps_done"], run[2]))
    assert got300[2]["steps_done"] < 300 and got300[2]["nfound"] == nev
    cpu300 = eref.eigenpairs_f64(K, None, eref.LARGEST, nev, 300, run=run)
    dv_cpu, dv_dev = float(np.max(np.abs(cpu300[0] - lam_w))) / norm, float(np.max(np.abs(got300[0] - lam_w))) / norm
    print("kernel n=1024 300 steps: values d_cpu=%.3e d_dev=%.3e" % (dv_cpu, dv_dev))
    assert dv_dev <= ref.tolerance(dv_cpu, n)


# ---- 4. no ghosts -----------------------------------------------------------------------------------------------------------------
def test_no_ghosts(gpu_pkg):
    n, steps, nev = 257, 64, 8
    A, lam = eref.outlier_matrix(n)
    want = lam[::-1][:nev]
    v0 = _start(n)
    cpu = eref.eigenpairs_f64(A, v0, eref.LARGEST, nev, steps)
    with _dense_solver(gpu_pkg, A) as s:
        vals, X, info = s.eigenpairs(nev, "largest", steps)
        alpha, beta, done = s.lanczos(v0[None, :], steps)         # the plain recurrence beside it: a record, not an assertion
    m = int(done[0])
    theta, weight = np.zeros(m), np.zeros(m)
    dp = gpu_pkg.cgx._dp
    assert gpu_pkg.cgx.lib().cgx_tridiag_quadrature(m, dp(np.ascontiguousarray(alpha[0, :m])), dp(np.ascontiguousarray(beta[0, :m])),
                                                     dp(theta), dp(weight)) == 0
    print("plain recurrence (cgx_lanczos + cgx_tridiag_quadrature), 12 largest Ritz values:", theta[-12:])
    print("copies of 17 in the plain recurrence: %d; with reorthogonalisation: %d" % (np.sum(np.abs(theta - 17.0) < 1e-6),
                                                                                      np.sum(np.abs(vals - 17.0) < 1e-6)))
    d_cpu, d_dev = float(np.max(np.abs(cpu[0] - want))) / 17.0, float(np.max(np.abs(vals - want))) / 17.0
    print("outliers: d_cpu=%.3e d_dev=%.3e" % (d_cpu, d_dev))
    assert d_dev <= ref.tolerance(d_cpu, n), (vals, want)         # the eight outliers, once each


# ---- 5. invariant subspaces -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [256, 1000])
@pytest.mark.parametrize("nd", [4, 8])
def test_invariant_subspaces(gpu_pkg, nd, n):
    steps, nev = 30, 8
    d = np.linspace(1.0, 9.0, nd)
    A, H, _ = ref.householder_matrix(n, d, 40 + nd)
    v0 = _start(n)
    cpu = eref.eigenpairs_f64(A, v0, eref.LARGEST, nev, steps)
    want = np.concatenate([d[::-1], np.zeros(nev)])[:nev]
    with _dense_solver(gpu_pkg, A) as s:
        vals, X, info = s.eigenpairs(nev, "largest", steps)
        one = s.eigenpairs(1, "largest", steps, v0=H[:, 1])       # an eigenvector start: one step
    assert info["steps_done"] == nd and info["nfound"] == min(nev, nd), info
    nf = info["nfound"]
    d_cpu, d_dev = float(np.max(np.abs(cpu[0] - want))) / 9.0, float(np.max(np.abs(vals - want))) / 9.0
    print("H D H nd=%d n=%d: values d_cpu=%.3e d_dev=%.3e" % (nd, n, d_cpu, d_dev))
    assert d_dev <= ref.tolerance(d_cpu, n)
    assert np.all(vals[nf:] == 0.0) and np.all(X[nf:] == 0.0) and np.all(info["residual"][nf:] == 0.0) and np.all(info["estimate"][nf:] == 0.0)
    assert np.max(info["residual"][:nf]) / 9.0 <= ref.tolerance(np.max(cpu[2]["residual"]) / 9.0, n)
    assert one[2]["steps_done"] == 1 and one[2]["nfound"] == 1
    assert abs(one[0][0] - d[1 % nd]) / 9.0 <= ref.tolerance(0.0, n)
    assert float(np.linalg.norm(eref.align(one[1][0], H[:, 1])[0] - H[:, 1])) <= ref.tolerance(0.0, n)


# ---- 6. tol -----------------------------------------------------------------------------------------------------------------------
def test_tol_stops_at_32_steps(gpu_pkg):
    K, lam, _, run = _kernel_case()
    with _dense_solver(gpu_pkg, K) as s:
        vt, Xt, it = s.eigenpairs(4, "largest", 200, tol=1e-10)
        v0, X0, i0 = s.eigenpairs(4, "largest", 32)
        v16, _, i16 = s.eigenpairs(4, "largest", 16)
    scale = float(lam[-1])
    print("tol: steps_done %d; estimates / ||A|| at 16 steps %.3e, at 32 steps %.3e" % (it["steps_done"], np.max(i16["estimate"]) / scale,
                                                                                      np.max(i0["estimate"]) / scale))
    assert it["steps_done"] == 32 and it["nfound"] == 4
    assert np.max(i16["estimate"]) > 1e-10 * scale and np.max(i0["estimate"]) <= 1e-10 * scale
    assert np.array_equal(vt, v0) and np.array_equal(Xt, X0)      # the bits of a tol = 0 run of 32 steps
    assert np.array_equal(it["residual"], i0["residual"]) and np.array_equal(it["estimate"], i0["estimate"])


# ---- 7. widths and edges ----------------------------------------------------------------------------------------------------------
def _same(o1, o2):
    return (np.array_equal(o1[0], o2[0]) and np.array_equal(o1[1], o2[1]) and o1[2]["steps_done"] == o2[2]["steps_done"] and
            o1[2]["nfound"] == o2[2]["nfound"] and np.array_equal(o1[2]["residual"], o2[2]["residual"]) and
            np.array_equal(o1[2]["estimate"], o2[2]["estimate"]))


@pytest.mark.parametrize("lda_pad", [-1, 0])
def test_widths(gpu_pkg, oracle, lda_pad):
    n, steps = 257, 257                                           # the full space: every wanted pair has converged
    A, lam, Qe, run = _hash_case(oracle, n)
    norm = float(np.max(np.abs(lam)))
    outs = {}
    with _hash_solver(gpu_pkg, n, lda_pad=lda_pad) as s:
        for nev in (1, 3, 8, 16):
            outs[nev] = s.eigenpairs(nev, "largest", steps)
        again = s.eigenpairs(8, "largest", steps)                 # a repeated call
        explicit = s.eigenpairs(8, "largest", steps, v0=_start(n))    # v0 = NULL against the explicit Rademacher vector
    with _hash_solver(gpu_pkg, n, lda_pad=lda_pad) as s:
        fresh = s.eigenpairs(8, "largest", steps)                 # a fresh context
    assert _same(outs[8], again) and _same(outs[8], explicit) and _same(outs[8], fresh)
    for nev in (1, 3, 8, 16):
        cpu = eref.eigenpairs_f64(A, None, eref.LARGEST, nev, steps, run=_cut(run, steps))
        lam_w, X_w = eref.wanted(lam, Qe, eref.LARGEST, nev)
        _compare("hash n=257 nev=%d lda_pad=%d" % (nev, lda_pad), n, norm, outs[nev], cpu, lam_w, X_w, A)
        # a pair does not depend on how many are asked for: the values are T's, the vector's chain is its own
        assert np.array_equal(outs[nev][0], outs[16][0][:nev]) and np.array_equal(outs[nev][1], outs[16][1][:nev])


@pytest.mark.parametrize("n", [1, 2])
def test_tiny_problems(gpu_pkg, n):
    A = np.array([[3.0]]) if n == 1 else np.array([[2.0, 1.0], [1.0, 2.0]])
    v0 = np.array([1.0]) if n == 1 else np.array([1.0, 0.0])
    want = np.array([3.0]) if n == 1 else np.array([3.0, 1.0])
    with _dense_solver(gpu_pkg, A) as s:
        vals, X, info = s.eigenpairs(n, "largest", n, v0=v0)
        small = s.eigenpairs(n, "smallest", n, v0=v0)
    assert info["steps_done"] == n and info["nfound"] == n
    floor = ref.tolerance(0.0, 4)                                 # the rule's floor (the restatement is exact here), ||A|| = 3
    assert np.max(np.abs(vals - want)) <= floor * 3.0 and np.max(np.abs(small[0] - want[::-1])) <= floor * 3.0
    for j in range(n):
        assert np.linalg.norm(A @ X[j] - vals[j] * X[j]) <= floor * 3.0 and abs(np.linalg.norm(X[j]) - 1.0) <= floor
    assert np.max(info["residual"]) <= floor * 3.0


# ---- 8. neighbours ----------------------------------------------------------------------------------------------------------------
def test_no_interference_with_the_other_paths(gpu_pkg):
    n = 2048
    B = np.random.default_rng(9).standard_normal((5, n))
    runs = []
    for with_eigs in (False, True):
        with gpu_pkg.CGSolver(gemv_variant=-1) as s:
            s.generate_lap2d_matrix(n)
            s.init_source_term(1.0 / n)
            s.set_max_iter(200)
            plan = s.gemv_plan()
            if with_eigs:
                vals, X, info = s.eigenpairs(5, "smallest", 40)
                assert np.all(np.isfinite(X)) and info["steps_done"] == 40
                assert s.gemv_plan() == plan
            x = np.zeros(n)
            r = s.solve(x)
            Xm, res = s.solve_multi(B)
            lz = s.lanczos(B, 20)
            Xf, inf = s.apply_function(B, gpu_pkg.cgx.FN_SQRT, 20)
            assert s.gemv_plan() == plan
            runs.append((x, r, Xm, res, lz, Xf, inf))
    (x1, r1, X1, res1, lz1, Xf1, inf1), (x2, r2, X2, res2, lz2, Xf2, inf2) = runs
    assert np.array_equal(x1, x2) and np.array_equal(X1, X2) and np.array_equal(Xf1, Xf2)
    assert all(np.array_equal(a, b) for a, b in zip(lz1, lz2))
    assert all(np.array_equal(inf1[k], inf2[k]) for k in ("steps_done", "change", "coef"))
    for key in ("iterations", "converged", "residual_prev", "residual_last", "x_norm", "rel_residual"):
        assert r1[key] == r2[key], key
        assert [q[key] for q in res1] == [q[key] for q in res2], key


# ---- 9. refusals ------------------------------------------------------------------------------------------------------------------
def _refused(cgx, status, call, needle=None):
    with pytest.raises(cgx.CgxError) as e:
        call()
    assert e.value.status == status, e.value
    if needle is not None:
        assert needle in str(e.value), e.value


def _still_solves(s, n):
    s.init_source_term(1.0 / n)
    s.set_max_iter(5)
    x = np.zeros(n)
    assert s.solve(x)["iterations"] >= 1 and np.all(np.isfinite(x))


def test_refusals(gpu_pkg):
    cgx = gpu_pkg.cgx
    L = cgx.lib()
    n = 1100
    # CGX_ERR_UNSUPPORTED: loopback ranks, banded and CSR storage, a preconditioner that is set
    for kw in (dict(comm_mode=cgx.COMM_LOOPBACK, nranks=2), dict(matrix_format=cgx.MATRIX_BANDED), dict(matrix_format=cgx.MATRIX_CSR)):
        with gpu_pkg.CGSolver(gemv_variant=-1, **kw) as s:
            s.generate_lap2d_matrix(n)
            _refused(cgx, ERR_UNSUPPORTED, lambda: s.eigenpairs(2, "largest", 4))
            _refused(cgx, ERR_UNSUPPORTED, lambda: s._probe_eigs_basis(np.ones(n), 4))
            _refused(cgx, ERR_UNSUPPORTED, lambda: s._probe_eigs_orthogonalise(np.ones((1, n)), np.ones(n)))
            _still_solves(s, n)
    with gpu_pkg.CGSolver(gemv_variant=-1) as s:
        vals = np.zeros(2)
        dp = cgx._dp
        call = L.cgx_eigenpairs
        assert call(s._h, 0, 2, 4, 0.0, None, 1, dp(vals), None, 0, None, None, None, None) == ERR_BAD_ARG     # no matrix
        s.generate_lap2d_matrix(n)
        for kind in ("jacobi", "pivchol"):
            s.set_preconditioner(kind)
            _refused(cgx, ERR_UNSUPPORTED, lambda: s.eigenpairs(2, "largest", 4), "preconditioner")
        s.set_preconditioner(None)
        ref_out = s.eigenpairs(2, "largest", 4)

        def good(k):
            assert _same(s.eigenpairs(2, "largest", 4), ref_out), k

        bad_calls = [
            lambda: s.eigenpairs(2, "largest", 0),
            lambda: s.eigenpairs(2, "largest", n + 1),                        # steps > n (and above the maximum)
            lambda: s.eigenpairs(2, "largest", cgx.MAX_LANCZOS_STEPS + 1),    # <= n, above the maximum
            lambda: s.eigenpairs(2, 2, 4),                                    # which unknown
            lambda: s.eigenpairs(2, -1, 4),
            lambda: s.eigenpairs(0, "largest", 4),
            lambda: s.eigenpairs(17, "largest", 40),
            lambda: s.eigenpairs(5, "largest", 4),                            # nev > steps
            lambda: s.eigenpairs(2, "largest", 4, tol=-1e-3),
            lambda: s.eigenpairs(2, "largest", 4, tol=np.nan),
            lambda: s.eigenpairs(2, "largest", 4, tol=np.inf),
        ]
        for k, bad in enumerate(bad_calls):
            _refused(cgx, ERR_BAD_ARG, bad)
            good(k)
        X = np.zeros((2, n))
        assert call(s._h, 0, 2, 4, 0.0, None, 1, None, dp(X), n, None, None, None, None) == ERR_BAD_ARG        # null values
        assert call(s._h, 0, 2, 4, 0.0, None, 1, dp(vals), dp(X), n - 1, None, None, None, None) == ERR_BAD_ARG  # ldv < n
        assert np.all(X == 0.0) and np.all(vals == 0.0)
        assert call(s._h, 0, 2, 4, 0.0, None, 1, dp(vals), None, 0, None, None, None, None) == 0               # the optional outputs may be NULL
        assert np.array_equal(vals, ref_out[0])
        good("raw")
        # a start vector of norm 0 or not finite: refused from the device, nothing is written
        for fill in (0.0, np.nan, np.inf):
            v0 = np.ones(n)
            v0[3] = fill
            if fill == 0.0:
                v0[:] = 0.0
            vals7 = np.full(2, 7.0)
            st = call(s._h, 0, 2, 4, 0.0, dp(v0), 1, dp(vals7), None, 0, None, None, None, None)
            assert st == ERR_BAD_ARG and "start vector" in L.cgx_last_error(s._h).decode() and np.all(vals7 == 7.0)
            good(fill)
        # the probes' own argument errors
        _refused(cgx, ERR_BAD_ARG, lambda: s._probe_eigs_basis(np.ones(n), 0))
        _refused(cgx, ERR_BAD_ARG, lambda: s._probe_eigs_orthogonalise(np.ones((1, n)), np.ones(n), 0))
        assert L.cgx_probe_eigs_orthogonalise(s._h, cgx.MAX_LANCZOS_STEPS + 1, dp(X), n, dp(X), dp(X), dp(X)) == ERR_BAD_ARG
        assert L.cgx_probe_eigs_orthogonalise(s._h, 1, dp(X), n - 1, dp(X), dp(X), dp(X)) == ERR_BAD_ARG
        good("probes")
        _still_solves(s, n)


def test_fault_walk(gpu_pkg):
    cgx = gpu_pkg.cgx
    n, steps = 600, 4

    def run(s):
        return s.eigenpairs(3, "smallest", steps)

    with gpu_pkg.CGSolver(gemv_variant=-1) as s:
        s.generate_lap2d_matrix(n)
        want = run(s)
    with gpu_pkg.CGSolver(gemv_variant=-1) as s:               # a fresh context: the walk also steps over the side block's making
        s.generate_lap2d_matrix(n)
        calls = 0
        while True:
            s._set_fault_after(calls)
            try:
                got = run(s)
            except cgx.CgxError as e:
                assert e.status == ERR_HIP, (calls, e)
                calls += 1
                assert calls < 200
                continue
            s._set_fault_after(-1)
            break
        # at least the calls of a call whose side block exists: the device, the upload, the set-up, six launches per step, four for
        # the read, then two uploads, the combine, K1m, the norms, two downloads and the synchronisation
        assert calls >= 1 + 2 + 6 * steps + 4 + 8, calls
        assert _same(got, want)
        assert _same(run(s), want)
        _still_solves(s, n)


# ---- 10. the command line ---------------------------------------------------------------------------------------------------------
def test_cli_eigs_prints_the_library_call(gpu_pkg, tmp_path):
    n, nev, steps = 1000, 4, 60
    exe = os.path.join(os.path.dirname(gpu_pkg.cgx.LIB_PATH), "cgsolver")
    out = tmp_path / "times.csv"
    r = subprocess.run([exe, str(n), str(out), "--eigs", "%d,%d" % (nev, steps)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    head = [ln for ln in r.stdout.splitlines() if "[EIGS]" in ln]
    assert len(head) == 1, r.stdout
    m = re.search(r"which = largest, nev = (\d+), steps = (\d+), steps_done = (\d+), nfound = (\d+)", head[0])
    assert m and (int(m.group(1)), int(m.group(2))) == (nev, steps), head[0]
    rows = [re.search(r"\[EIG (\d+)\] value = (\S+), residual = (\S+), estimate = (\S+)", ln) for ln in r.stdout.splitlines() if "[EIG " in ln]
    assert len(rows) == nev and all(rows), r.stdout
    assert out.read_text().startswith("%d,1," % n)
    with gpu_pkg.CGSolver(gemv_variant=-1) as s:
        s.generate_lap2d_matrix(n)
        vals, _, info = s.eigenpairs(nev, "largest", steps)
    assert (int(m.group(3)), int(m.group(4))) == (info["steps_done"], info["nfound"])
    for j, row in enumerate(rows):
        assert int(row.group(1)) == j and float(row.group(2)) == vals[j]                       # printed with 17 digits
        assert float(row.group(3)) == pytest.approx(info["residual"][j], rel=1e-10)            # printed with 12 digits
        assert float(row.group(4)) == pytest.approx(info["estimate"][j], rel=1e-10)
