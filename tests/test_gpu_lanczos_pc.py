"""cgx_lanczos_pc / cgx_precond_logdet / cgx_slq_probes / cgx_trace_slq_pc (csrc/cgx_lanczos_pc.hip) on the
MI355X.

- the coefficients and eta0^2 against a longdouble recurrence with full reorthogonalisation in the M-inner product, under the
  pivoted-Cholesky factor (the device's own L and delta) and under Jacobi;
- breakdown and exact quadrature on a matrix whose Jacobi-scaled form has four eigenvalues;
- the quadratures against dense references; log det M; the library's probes, determinism, permutations;
- the log det of a kernel matrix end to end, against the plain path's standard error;
- scope: no preconditioner, the row pitch, no interference, refusals, the fault walk, the command line.

The tolerance rule is section 17's (lanczos_reference.tolerance): wherever a device value is compared with a high-precision
reference, the test computes d_cpu, the deviation of the float64 numpy restatement of the same recurrence
(tests/lanczos_pc_reference.py) from that reference, and allows the device 16 max(d_cpu, n 2^-52).
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import lanczos_pc_reference as pref
import lanczos_reference as ref
import multi_pc_reference as mref
import pivchol_reference

pytestmark = pytest.mark.gpu

ERR_BAD_ARG, ERR_HIP, ERR_UNSUPPORTED = 1, 3, 7   # cgx_status (include/cgx.h)
ELL, SIGMA2 = 0.2, 1e-2
STEPS = 12
_CACHE = {}


def _kernel(n):
    return pivchol_reference.kernel_matrix(n, ELL, SIGMA2)[0]


def _kernel_solver(pkg, n, rank, **kw):
    s = pkg.CGSolver(gemv_variant=kw.pop("gemv_variant", -1), **kw)
    s.set_matrix_dense(_kernel(n))
    if rank:
        s.set_preconditioner("pivchol", rank=rank)
    return s


def _dense_solver(pkg, A, kind=None, **kw):
    s = pkg.CGSolver(gemv_variant=-1)
    s.set_matrix_dense(A)
    if kind:
        s.set_preconditioner(kind, **kw)
    return s


def _start_vectors(n):
    if ("v0", n) not in _CACHE:
        V0 = np.random.default_rng(2000 + n).standard_normal((16, n))
        V0.setflags(write=False)
        _CACHE[("v0", n)] = V0
    return _CACHE[("v0", n)]


def _longdouble(A):
    if ("ld", id(A)) not in _CACHE:
        _CACHE[("ld", id(A))] = (A, np.asarray(A, dtype=pref.LD))   # (A itself is kept so that its id stays its own)
    return _CACHE[("ld", id(A))][1]


def _references(key, A, V0, ap64, apld, steps=STEPS):
    """Made once per key and left unchanged: per start vector the longdouble reference and the float64 restatement."""
    if key not in _CACHE:
        Al = _longdouble(A)
        hi = [pref.lanczos_pc_longdouble(Al, apld, v, steps) for v in V0]
        cpu = [pref.lanczos_pc_f64(A, ap64, v, steps) for v in V0]
        out = tuple(np.array(x) for x in ([h[0] for h in hi], [h[1] for h in hi], [h[2] for h in hi], [c[0] for c in cpu],
                                          [c[1] for c in cpu], [c[2] for c in cpu], [c[3] for c in cpu]))
        for a in out:
            a.setflags(write=False)
        _CACHE[key] = out
    return _CACHE[key]


def _check_coefficients(tag, n, got, refs, nvec):
    alpha, beta, done, eta2 = got
    a_ref, b_ref, e_ref, a_cpu, b_cpu, m_cpu, e_cpu = refs
    assert list(done) == [STEPS] * nvec and list(m_cpu[:nvec]) == [STEPS] * nvec
    for j in range(nvec):
        scale = float(np.max(np.abs(a_ref[j])))
        d_cpu = float(max(np.max(np.abs(a_cpu[j] - a_ref[j])), np.max(np.abs(b_cpu[j] - b_ref[j])))) / scale
        d_dev = float(max(np.max(np.abs(alpha[j] - a_ref[j])), np.max(np.abs(beta[j] - b_ref[j])))) / scale
        e_c = float(abs(e_cpu[j] - e_ref[j]) / e_ref[j])
        e_d = float(abs(eta2[j] - e_ref[j]) / e_ref[j])
        print("%s nvec=%d column %d: d_cpu=%.3e d_dev=%.3e tol=%.3e; eta2: cpu %.3e dev %.3e" %
              (tag, nvec, j, d_cpu, d_dev, ref.tolerance(d_cpu, n), e_c, e_d))
        assert d_dev <= ref.tolerance(d_cpu, n), (tag, nvec, j, d_cpu, d_dev)
        assert e_d <= ref.tolerance(e_c, n), (tag, nvec, j, e_c, e_d)


# ---- 1. the coefficients ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,rank,nvec", [(1000, 64, 1), (1000, 64, 3), (1000, 64, 8), (1000, 64, 16), (1000, 16, 1), (1000, 16, 3),
                                         (1000, 16, 8), (1000, 16, 16), (1000, 5, 3), (257, 5, 3), (1000, 64, 2), (1000, 64, 5),
                                         (1000, 64, 9)])
def test_coefficients_pivchol(gpu_pkg, n, rank, nvec):
    A, V0 = _kernel(n), _start_vectors(n)
    with _kernel_solver(gpu_pkg, n, rank) as s:
        got = s.lanczos_pc(V0[:nvec], STEPS)
        _, L, delta = s._probe_precond_lowrank()              # the device's own factor
    refs = _references(("pc", n, rank), A, V0, pref.lowrank_apply(L, delta), pref.lowrank_apply(L, delta, pref.LD))
    _check_coefficients("pivchol n=%d rank=%d" % (n, rank), n, got, refs, nvec)


def _jacobi_matrix(oracle, n=1024):
    if ("jac", n) not in _CACHE:
        A = mref.scaled_lap2d(oracle.generate_lap2d(n))
        A.setflags(write=False)
        _CACHE[("jac", n)] = A
    return _CACHE[("jac", n)]


@pytest.mark.parametrize("nvec", [1, 3, 8, 16])
def test_coefficients_jacobi(gpu_pkg, oracle, nvec):
    n = 1024
    A, V0 = _jacobi_matrix(oracle, n), _start_vectors(n)
    with _dense_solver(gpu_pkg, A, "jacobi") as s:
        got = s.lanczos_pc(V0[:nvec], STEPS)
    refs = _references(("jc", n), A, V0, pref.jacobi_apply(A), pref.jacobi_apply(A, pref.LD))
    _check_coefficients("jacobi n=%d" % n, n, got, refs, nvec)


# ---- 2. breakdown and exact quadrature --------------------------------------------------------------------------------------------
def test_breakdown_and_exact_quadrature(gpu_pkg):
    n, steps, seed = 1000, 12, 1
    A, s_scale, vec, c, b00 = pref.breakdown_matrix(n)
    d = np.diag(A)
    ap = pref.jacobi_apply(A)
    with _dense_solver(gpu_pkg, A, "jacobi") as s:
        Z = s.slq_probes(gpu_pkg.cgx.SLQ_LOG, 8, seed)
        out = s.logdet_pc(probes=8, steps=steps, seed=seed)
        alpha, beta, done, eta2 = s.lanczos_pc(Z, steps)
        V = np.array([Z[0], np.sqrt(d) * vec[1], Z[1], Z[2]])  # an eigenvector start beside running companions
        alpha2, beta2, done2, _ = s.lanczos_pc(V, steps)
        alpha3, beta3, done3, _ = s.lanczos_pc(np.array([Z[0], Z[3], Z[1], Z[2]]), steps)   # the same width, no frozen companion
    assert np.array_equal(Z, pref.probes_log_jacobi(seed, 8, A))
    assert list(done) == [4] * 8, done
    assert list(done2) == [4, 1, 4, 4], done2
    assert np.all(alpha[:, 4:] == 0) and np.all(beta[:, 4:] == 0)
    assert np.all(alpha2[1, 1:] == 0) and np.all(beta2[1, 1:] == 0)
    a_cpu, _, m_cpu, _ = pref.lanczos_pc_f64(A, ap, V[1], steps)
    assert m_cpu == 1
    exact_a = 8.0 / b00                                        # the eigenvalue (1 + 7) / B_00 of v2
    print("eigenvector start: alpha_0 - exact = %.3e (float64 %.3e)" % (alpha2[1, 0] - exact_a, a_cpu[0] - exact_a))
    assert abs(alpha2[1, 0] - exact_a) <= ref.tolerance(abs(a_cpu[0] - exact_a) / exact_a, n) * exact_a
    for col, other in ((0, 0), (2, 2), (3, 3)):                # the running columns: the bits of a call without the frozen one
        assert np.array_equal(alpha2[col], alpha3[other]) and np.array_equal(beta2[col], beta3[other])
    for j in range(8):
        amax = np.max(np.abs(alpha[j]))
        assert beta[j, 3] <= ref.BREAK * amax and np.all(beta[j, :3] >= 2.0 ** -18 * amax), beta[j]
        g = Z[j] / np.sqrt(d)
        terms = pref.breakdown_log_terms(g, vec, c)
        exact, scale = float(terms.sum()), float(np.abs(terms).sum())
        ac, bc, mc, ec = pref.lanczos_pc_f64(A, ap, Z[j], steps)
        assert mc == 4
        d_cpu = abs(ref.quadrature(ac, bc, mc, ec, np.log) - exact) / scale
        d_dev = abs(out["per_probe"][j] - exact) / scale
        print("breakdown matrix probe %d: d_cpu=%.3e d_dev=%.3e (scale %.3f)" % (j, d_cpu, d_dev, scale))
        assert d_dev <= ref.tolerance(d_cpu, n), (j, d_cpu, d_dev)
    logs = np.log(d.astype(pref.LD))
    assert abs(out["logdet_precond"] - float(logs.sum())) <= n * 2.0 ** -53 * float(np.sum(np.abs(logs)))   # the bound of section 4


# ---- 3. quadrature against dense references ---------------------------------------------------------------------------------------
def test_log_quadrature_against_eigh(gpu_pkg):
    """per_probe against g^T log(G^-1 A G^-T) g by numpy.linalg.eigh, M = G G^T from the device's L and delta, g = G^-1 z.  The
    device applies M^-1 through the explicit inverse of delta I + L^T L that the set-up keeps, and so does the float64
    restatement (lanczos_pc_reference.lowrank_apply): that inverse, not the recurrence, sets the level of both deviations."""
    n, rank, steps = 1000, 64, 24
    A = _kernel(n)
    with _kernel_solver(gpu_pkg, n, rank) as s:
        s.precond_logdet()                                    # makes the factor
        _, L, delta = s._probe_precond_lowrank()
        Z = pref.probes_log_lowrank(11, 8, L, delta)          # caller probes of covariance M
        out = s.logdet_pc(steps=steps, Z=Z)
    M = L @ L.T + delta * np.eye(n)
    Gi = np.linalg.inv(np.linalg.cholesky(M))
    lam, Q = np.linalg.eigh(Gi @ A @ Gi.T)
    C2 = ((Gi @ Z.T).T @ Q) ** 2
    ap = pref.lowrank_apply(L, delta)
    for j in range(8):
        exact = float(C2[j] @ np.log(lam))
        a, b, m, e2 = pref.lanczos_pc_f64(A, ap, Z[j], steps)
        d_cpu = abs(ref.quadrature(a, b, m, e2, np.log) - exact) / abs(exact)
        d_dev = abs(out["per_probe"][j] - exact) / abs(exact)
        print("kernel matrix, log, probe %d: exact %.6f d_cpu=%.3e d_dev=%.3e" % (j, exact, d_cpu, d_dev))
        assert d_dev <= ref.tolerance(d_cpu, n), (j, d_cpu, d_dev)
    assert lam[0] * (1 - 1e-6) <= out["ritz_min"] and out["ritz_max"] <= lam[-1] * (1 + 1e-6)


def test_inverse_quadrature_against_solve(gpu_pkg):
    n, rank, steps, seed = 1024, 64, 40, 4
    A = _kernel(n)
    Z = ref.rademacher(seed, 8, n)
    with _kernel_solver(gpu_pkg, n, rank) as s:
        out = s.trace_inv_pc(probes=8, steps=steps, seed=seed)
        _, L, delta = s._probe_precond_lowrank()
    assert out["logdet_precond"] == 0.0
    X = np.linalg.solve(A, Z.T).T
    ap = pref.lowrank_apply(L, delta)
    for j in range(8):
        exact = float(Z[j] @ X[j])
        a, b, m, e2 = pref.lanczos_pc_f64(A, ap, Z[j], steps)
        d_cpu = abs(ref.quadrature(a, b, m, e2, lambda t: 1.0 / t) - exact) / abs(exact)
        d_dev = abs(out["per_probe"][j] - exact) / abs(exact)
        print("kernel matrix, 1/x, probe %d: d_cpu=%.3e d_dev=%.3e" % (j, d_cpu, d_dev))
        assert d_dev <= ref.tolerance(d_cpu, n), (j, d_cpu, d_dev)


# ---- 4. log det M -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rank", [5, 16, 64])
def test_precond_logdet_pivchol(gpu_pkg, rank):
    """Against (n - k) log delta + log det(delta I + L^T L) in longdouble from the device's L and delta.  The library takes the
    second term from the device's float64 inverse of C = delta I + L^T L: an inverse computed in float64 is off by about cond(C)
    2^-52 relative, and log det moves by tr(C dC^-1) <= k times that; the bound gives the inversion and the host factorisation 16
    times it, plus the rounding of the k + 1 logarithms and of their sum."""
    n = 1000
    with _kernel_solver(gpu_pkg, n, rank) as s:
        got = s.precond_logdet()
        again = s.precond_logdet()
        _, L, delta = s._probe_precond_lowrank()
    Ll = L.astype(pref.LD)
    Cl = Ll.T @ Ll + pref.LD(delta) * np.eye(rank, dtype=pref.LD)
    R = pivchol_reference._chol_factor(Cl)
    exact = (n - rank) * np.log(pref.LD(delta)) + 2 * np.sum(np.log(np.diag(R)))
    cond = float(np.linalg.cond(Cl.astype(np.float64)))
    bound = 16 * rank * cond * ref.EPS + (rank + 2) * ref.EPS * (abs(float(exact)) + (n - rank) * abs(np.log(delta)))
    print("log det M rank %d: device %.12f longdouble %.12f, off by %.3e (bound %.3e, cond C %.3e)" %
          (rank, got, float(exact), abs(got - float(exact)), bound, cond))
    assert got == again
    assert abs(got - float(exact)) <= bound


def test_precond_logdet_jacobi(gpu_pkg, oracle):
    n = 1024
    A = _jacobi_matrix(oracle, n)
    logs = np.log(np.diag(A).astype(pref.LD))
    with _dense_solver(gpu_pkg, A, "jacobi") as s:
        got = s.precond_logdet()
        s.set_preconditioner(None)
        assert s.precond_logdet() == 0.0
    bound = n * 2.0 ** -53 * float(np.sum(np.abs(logs)))
    print("log det D: device %.12f longdouble %.12f, off by %.3e (bound %.3e)" % (got, float(logs.sum()), abs(got - float(logs.sum())), bound))
    assert abs(got - float(logs.sum())) <= bound


# ---- 5. the probes ----------------------------------------------------------------------------------------------------------------
def _same(o1, o2):
    return all(np.array_equal(o1[k], o2[k]) for k in ("estimate", "std_error", "per_probe", "ritz_min", "ritz_max", "logdet_precond"))


def test_library_probes_and_determinism(gpu_pkg):
    n, rank, probes, steps, seed = 1000, 16, 11, 16, 77
    cgx = gpu_pkg.cgx
    perm = np.array([5, 2, 7, 0, 1, 6, 3, 4, 10, 8, 9])      # within the batches of 8 and 3
    with _kernel_solver(gpu_pkg, n, rank) as s:
        Z = s.slq_probes(cgx.SLQ_LOG, probes, seed)
        Zi = s.slq_probes(cgx.SLQ_INV, probes, seed)
        _, L, delta = s._probe_precond_lowrank()
        lib = s.logdet_pc(probes=probes, steps=steps, seed=seed)   # batches of 8 + 3
        own = s.logdet_pc(steps=steps, Z=Z)
        again = s.logdet_pc(probes=probes, steps=steps, seed=seed)
        other = s.logdet_pc(probes=probes, steps=steps, seed=seed + 1)
        shuffled = s.logdet_pc(steps=steps, Z=Z[perm])
        inv_lib = s.trace_inv_pc(probes=probes, steps=steps, seed=seed)
        inv_own = s.trace_inv_pc(steps=steps, Z=Zi)
    want = pref.probes_log_lowrank(seed, probes, L, delta)
    bound = (rank + 2) * 2.0 ** -53 * (np.sum(np.abs(L), axis=1) + np.sqrt(delta))
    print("probes: max |dz| / bound = %.3f" % float(np.max(np.abs(Z - want) / bound[None, :])))
    assert np.all(np.abs(Z - want) <= bound[None, :])
    assert np.array_equal(Zi, ref.rademacher(seed, probes, n))
    assert _same(lib, own) and _same(lib, again) and _same(inv_lib, inv_own)
    assert not np.array_equal(lib["per_probe"], other["per_probe"])
    assert np.array_equal(shuffled["per_probe"], own["per_probe"][perm])
    assert abs(lib["std_error"] - np.std(lib["per_probe"], ddof=1) / np.sqrt(probes)) <= 1e-12 * lib["std_error"]
    assert abs(lib["estimate"] - (lib["logdet_precond"] + np.mean(lib["per_probe"]))) <= 1e-14 * abs(lib["estimate"])
    assert abs(inv_lib["estimate"] - np.mean(inv_lib["per_probe"])) <= 1e-14 * abs(inv_lib["estimate"])


# ---- 6. end to end ----------------------------------------------------------------------------------------------------------------
def test_logdet_of_a_kernel_matrix(gpu_pkg):
    """16 library probes of 24 steps through a rank-64 factor against numpy.linalg.slogdet, and against the plain path's standard
    error at 100 steps.  The float64 restatement with the restated library probes of seed 1 (factor by
    pivchol_reference.pivoted_cholesky) is 1.1 standard errors off and has a standard error of 2.35 against the plain path's 16.07."""
    n, rank = 1024, 64
    A = _kernel(n)
    sign, exact = np.linalg.slogdet(A)
    assert sign == 1.0
    with _kernel_solver(gpu_pkg, n, rank) as s:
        out = s.logdet_pc(probes=16, steps=24, seed=1)
        s.set_preconditioner(None)
        plain = s.logdet(probes=16, steps=100, seed=1)
    print("kernel matrix: estimate %.6f slogdet %.6f, %.2f standard errors; std_error %.3f against the plain path's %.3f; log det M %.6f; "
          "Ritz values in [%.4f, %.4f]" % (out["estimate"], exact, abs(out["estimate"] - exact) / out["std_error"], out["std_error"],
                                           plain["std_error"], out["logdet_precond"], out["ritz_min"], out["ritz_max"]))
    assert abs(out["estimate"] - exact) <= 3 * out["std_error"]
    assert out["std_error"] < plain["std_error"]


# ---- 7. scope ---------------------------------------------------------------------------------------------------------------------
def test_no_preconditioner_is_the_plain_path(gpu_pkg):
    n = 1000
    V0 = _start_vectors(n)[:3]
    with _kernel_solver(gpu_pkg, n, 0) as s:
        a, b, done = s.lanczos(V0, STEPS)
        a2, b2, done2, eta2 = s.lanczos_pc(V0, STEPS)
        plain = s.logdet(probes=9, steps=STEPS, seed=3)
        pc = s.logdet_pc(probes=9, steps=STEPS, seed=3)
        assert s.precond_logdet() == 0.0
        Z = s.slq_probes(gpu_pkg.cgx.SLQ_LOG, 9, 3)
    assert np.array_equal(a, a2) and np.array_equal(b, b2) and np.array_equal(done, done2)
    assert np.all(np.abs(eta2 - np.sum(V0 * V0, axis=1)) <= n * ref.EPS * eta2)
    assert all(np.array_equal(plain[k], pc[k]) for k in plain) and pc["logdet_precond"] == 0.0
    assert np.array_equal(Z, ref.rademacher(3, 9, n))


@pytest.mark.parametrize("kind", ["pivchol", "jacobi"])
def test_row_pitch_without_pad_columns(gpu_pkg, kind):
    n = 1024
    A, V0 = _kernel(n), _start_vectors(n)[:5]
    got = []
    for kw in ({}, {"lda_pad": 0}):
        with gpu_pkg.CGSolver(gemv_variant=-1, **kw) as s:
            s.set_matrix_dense(A)
            s.set_preconditioner(kind, rank=16) if kind == "pivchol" else s.set_preconditioner(kind)
            o = s.logdet_pc(probes=9, steps=8, seed=2)
            got.append(s.lanczos_pc(V0, 8) + (o["per_probe"], np.array([o["estimate"], o["logdet_precond"]])))
    assert all(np.array_equal(x, y) for x, y in zip(*got))


def test_no_interference_with_the_solves(gpu_pkg):
    n = 1024
    A, b = pivchol_reference.kernel_matrix(n, ELL, SIGMA2)
    B = mref.rhs_block(A, b, 5)
    runs = []
    for with_logdet in (False, True):
        with _kernel_solver(gpu_pkg, n, 16) as s:
            s.set_source_term(b)
            s.set_max_iter(60)
            s.tolerance(1e-6 * float(np.linalg.norm(b)))
            plan = s.gemv_plan()
            if with_logdet:
                out = s.logdet_pc(probes=9, steps=10)
                assert np.isfinite(out["estimate"]) and out["ritz_min"] > 0
                assert s.gemv_plan() == plan
            x = np.zeros(n)
            r = s.solve(x)
            X, res = s.solve_multi_pc(B)
            assert s.gemv_plan() == plan
            runs.append((x, r, X, res))
    (x1, r1, X1, res1), (x2, r2, X2, res2) = runs
    assert np.array_equal(x1, x2) and np.array_equal(X1, X2)
    for key in ("iterations", "converged", "residual_prev", "residual_last", "x_norm", "rel_residual"):
        assert r1[key] == r2[key], key
        assert [q[key] for q in res1] == [q[key] for q in res2], key


def _refused(cgx, status, call, needle=None):
    with pytest.raises(cgx.CgxError) as e:
        call()
    assert e.value.status == status, e.value
    if needle is not None:
        assert needle in str(e.value), e.value
    return str(e.value)


def _still_solves(s, n):
    s.set_preconditioner(None)
    s.init_source_term(1.0 / n)
    s.set_max_iter(5)
    x = np.zeros(n)
    assert s.solve(x)["iterations"] >= 1 and np.all(np.isfinite(x))


def test_refusals(gpu_pkg):
    cgx = gpu_pkg.cgx
    L = cgx.lib()
    n = 1024
    V = np.ones((2, n))
    V[1, ::2] = -1.0

    def calls(s):
        return (lambda: s.lanczos_pc(V, 4), lambda: s.logdet_pc(probes=2, steps=4), lambda: s.trace_inv_pc(probes=2, steps=4),
                lambda: s.slq_probes(cgx.SLQ_LOG, 2), lambda: s.precond_logdet())

    # several ranks / loopback, banded and CSR storage: cgx_solve_multi_pc's status and words
    for kw in (dict(comm_mode=cgx.COMM_LOOPBACK, nranks=2), dict(matrix_format=cgx.MATRIX_BANDED), dict(matrix_format=cgx.MATRIX_CSR)):
        for kind in (None, "jacobi"):
            with gpu_pkg.CGSolver(gemv_variant=-1, **kw) as s:
                s.generate_lap2d_matrix(n)
                s.set_preconditioner(kind)
                with pytest.raises(cgx.CgxError) as e:
                    s.solve_multi_pc(V)
                want = str(e.value)
                for call in calls(s):
                    msg = _refused(cgx, ERR_UNSUPPORTED, call)
                    assert re.sub(r"cgx_\w+:", "cgx_solve_multi_pc:", msg, count=1) == want, (msg, want)
                _still_solves(s, n)
    with gpu_pkg.CGSolver(gemv_variant=-1) as s:
        s.generate_lap2d_matrix(n)
        s.set_preconditioner("jacobi", block=8)               # block Jacobi
        for call in calls(s):
            _refused(cgx, ERR_UNSUPPORTED, call, "block Jacobi")
        for kind in ("jacobi", "pivchol"):                    # the plain entry points keep refusing a preconditioner
            s.set_preconditioner(kind)
            _refused(cgx, ERR_UNSUPPORTED, lambda: s.lanczos(V, 4), "preconditioner")
            _refused(cgx, ERR_UNSUPPORTED, lambda: s.logdet(probes=2, steps=4), "preconditioner")
        s.set_preconditioner("jacobi")
        ref_out = s.lanczos_pc(V, 4)
        bad_calls = [
            lambda: s.lanczos_pc(np.ones((0, n)), 4),
            lambda: s.lanczos_pc(np.ones((17, n)), 4),
            lambda: s.lanczos_pc(V, 0),
            lambda: s.lanczos_pc(V, n + 1),
            lambda: s.logdet_pc(probes=0, steps=4),
            lambda: s.logdet_pc(probes=cgx.MAX_PROBES + 1, steps=4),
            lambda: s.logdet_pc(probes=2, steps=0),
            lambda: s.logdet_pc(probes=2, steps=cgx.MAX_LANCZOS_STEPS + 1),
            lambda: s._trace_slq_pc(2, 2, 4, 1, None),        # unknown fn
            lambda: s.slq_probes(2, 2),
            lambda: s.slq_probes(cgx.SLQ_LOG, 0),
            lambda: s.slq_probes(cgx.SLQ_LOG, cgx.MAX_PROBES + 1),
        ]
        for k, call in enumerate(bad_calls):
            _refused(cgx, ERR_BAD_ARG, call)
            assert all(np.array_equal(x, y) for x, y in zip(s.lanczos_pc(V, 4), ref_out)), k
        a, b, e2 = np.zeros((2, 4)), np.zeros((2, 4)), np.zeros(2)
        done = (C.c_int * 2)()
        est, err = C.c_double(), C.c_double()
        dp = cgx._dp
        assert L.cgx_lanczos_pc(s._h, 2, 4, dp(V), n - 1, dp(a), dp(b), done, dp(e2)) == ERR_BAD_ARG      # ldv < n
        assert L.cgx_lanczos_pc(s._h, 2, 4, None, n, dp(a), dp(b), done, dp(e2)) == ERR_BAD_ARG           # null pointers
        assert L.cgx_lanczos_pc(s._h, 2, 4, dp(V), n, None, dp(b), done, dp(e2)) == ERR_BAD_ARG
        assert L.cgx_lanczos_pc(s._h, 2, 4, dp(V), n, dp(a), None, done, dp(e2)) == ERR_BAD_ARG
        assert L.cgx_lanczos_pc(s._h, 2, 4, dp(V), n, dp(a), dp(b), None, dp(e2)) == ERR_BAD_ARG
        assert L.cgx_lanczos_pc(s._h, 2, 4, dp(V), n, dp(a), dp(b), done, None) == ERR_BAD_ARG
        assert L.cgx_trace_slq_pc(s._h, 0, 2, 4, 1, dp(V), n - 1, C.byref(est), C.byref(err), None, None, None) == ERR_BAD_ARG
        assert L.cgx_trace_slq_pc(s._h, 0, 2, 4, 1, None, 0, None, C.byref(err), None, None, None) == ERR_BAD_ARG
        assert L.cgx_trace_slq_pc(s._h, 0, 2, 4, 1, None, 0, C.byref(est), None, None, None, None) == ERR_BAD_ARG
        assert L.cgx_slq_probes(s._h, 0, 2, 1, None, n) == ERR_BAD_ARG
        assert L.cgx_slq_probes(s._h, 0, 2, 1, dp(V), n - 1) == ERR_BAD_ARG
        assert L.cgx_precond_logdet(s._h, None) == ERR_BAD_ARG
        for kind in ("jacobi", "pivchol"):                    # a bad start vector names its column
            s.set_preconditioner(kind)
            good = s.lanczos_pc(V, 4)
            for fill in (0.0, np.nan, np.inf):
                W = np.ones((3, n))
                W[1] = fill
                _refused(cgx, ERR_BAD_ARG, lambda: s.lanczos_pc(W, 4), "start vector 1")
                Wp = np.ones((10, n))
                Wp[9] = fill
                _refused(cgx, ERR_BAD_ARG, lambda: s.logdet_pc(steps=4, Z=Wp), "start vector 9")
                assert all(np.array_equal(x, y) for x, y in zip(s.lanczos_pc(V, 4), good))
        _still_solves(s, n)
    for kind in ("jacobi", "pivchol"):                        # the persistent kernels: the single solve's status and message
        with gpu_pkg.CGSolver(gemv_variant=40000) as s:
            s.generate_lap2d_matrix(n)
            s.init_source_term(1.0 / n)
            s.set_preconditioner(kind)
            with pytest.raises(cgx.CgxError) as e:
                s.solve(np.zeros(n))
            for call in calls(s):
                assert _refused(cgx, ERR_UNSUPPORTED, call) == str(e.value)
    with gpu_pkg.CGSolver(gemv_variant=10825) as s:            # a K1 shape with split columns
        s.generate_lap2d_matrix(n)
        s.set_preconditioner("pivchol", rank=8)
        for call in calls(s):
            _refused(cgx, ERR_UNSUPPORTED, call, "split columns")
    with gpu_pkg.CGSolver(gemv_variant=-1) as s:               # rank > n
        s.generate_lap2d_matrix(100)
        s.set_preconditioner("pivchol", rank=101)
        V100 = np.ones((2, 100))
        _refused(cgx, ERR_BAD_ARG, lambda: s.lanczos_pc(V100, 4), "rank 101")
        _refused(cgx, ERR_BAD_ARG, lambda: s.logdet_pc(probes=2, steps=4), "rank 101")
        _still_solves(s, 100)


def test_a_matrix_that_is_not_positive_definite(gpu_pkg):
    cgx = gpu_pkg.cgx
    n = 1024
    A = _kernel(n)
    bad = np.array(A)
    bad[321, 321] = -1.0e6
    with gpu_pkg.CGSolver(gemv_variant=-1) as s:               # the set-up's refusal: a diagonal entry
        s.set_matrix_dense(bad)
        for kind in ("pivchol", "jacobi"):
            s.set_preconditioner(kind, rank=16) if kind == "pivchol" else s.set_preconditioner(kind)
            _refused(cgx, ERR_BAD_ARG, lambda: s.logdet_pc(probes=2, steps=6), "row 321")
            _refused(cgx, ERR_BAD_ARG, lambda: s.lanczos_pc(np.ones((2, n)), 6), "row 321")
        s.set_matrix_dense(A)
        s.set_preconditioner("pivchol", rank=16)
        got = s.logdet_pc(probes=3, steps=6)
    with _kernel_solver(gpu_pkg, n, 16) as s:
        assert _same(s.logdet_pc(probes=3, steps=6), got)
    m = 256                                                    # an indefinite matrix with a positive diagonal: a Ritz value <= 0
    Aind = np.diag(np.full(m, 2.0))
    Aind[16, 17] = Aind[17, 16] = 5.0                          # D^-1/2 A D^-1/2 has the eigenvalues 1, 3.5 and, along e16 - e17, -1.5
    Z = np.tile(np.where(np.arange(m) % 2 == 0, 1.0, -1.0), (2, 1))   # parts along e16 - e17 and in the eigenspace of 1: m = 2
    Z[1, :8] = 1.0
    with _dense_solver(gpu_pkg, Aind, "jacobi") as s:
        _refused(cgx, ERR_BAD_ARG, lambda: s.logdet_pc(steps=6, Z=np.sqrt(2.0) * Z), "matrix is not positive definite")
        assert "-1.5" in cgx.lib().cgx_last_error(s._h).decode()   # the Ritz value
        _refused(cgx, ERR_BAD_ARG, lambda: s.trace_inv_pc(steps=6, Z=Z), "matrix is not positive definite")
        alpha, beta, done, _ = s.lanczos_pc(Z, 6)              # the recurrence itself takes any symmetric matrix
        assert list(done) == [2, 2] and np.all(alpha[:, 2:] == 0)
        _still_solves(s, m)


@pytest.mark.parametrize("entry", ["lanczos_pc", "logdet_pc"])
@pytest.mark.parametrize("kind", ["pivchol", "jacobi"])
def test_fault_walk(gpu_pkg, kind, entry):
    """Every runtime call of one cgx_lanczos_pc / one cgx_trace_slq_pc fails once, through the existing error-path hook
    (cgx_probe_set_fault_after: the call is not made and reports a failure; nothing on the device is made to fail)."""
    cgx = gpu_pkg.cgx
    n, steps, rank = 600, 4, 8
    A = _kernel(n)
    V = _start_vectors(n)[:3]

    def make():
        s = gpu_pkg.CGSolver(gemv_variant=-1)
        s.set_matrix_dense(A)
        s.set_preconditioner(kind, rank=rank) if kind == "pivchol" else s.set_preconditioner(kind)
        return s

    def run(s):
        if entry == "lanczos_pc":
            return s.lanczos_pc(V, steps)
        o = s.logdet_pc(probes=10, steps=steps, seed=3)       # two batches
        return o["per_probe"], np.array([o["estimate"], o["std_error"], o["ritz_min"], o["ritz_max"], o["logdet_precond"]])

    with make() as s:
        want = run(s)
    with make() as s:                                          # a fresh context: the walk also steps over the set-up and the side block
        calls = 0
        while True:
            s._set_fault_after(calls)
            try:
                got = run(s)
            except cgx.CgxError as e:
                assert e.status == ERR_HIP, (calls, e)
                calls += 1
                assert calls < 400
                continue
            s._set_fault_after(-1)
            break
        assert calls >= (2 * steps + 6) * (1 if entry == "lanczos_pc" else 2), calls
        assert all(np.array_equal(a, b) for a, b in zip(got, want))
        assert all(np.array_equal(a, b) for a, b in zip(run(s), want))
        _still_solves(s, n)


def test_cli_logdet_pc_prints_the_library_call(gpu_pkg, tmp_path):
    n, probes, steps = 1024, 8, 20
    exe = os.path.join(os.path.dirname(gpu_pkg.cgx.LIB_PATH), "cgsolver")
    out = tmp_path / "times.csv"
    r = subprocess.run([exe, str(n), str(out), "--pivchol", "16", "--logdet-pc", "%d,%d" % (probes, steps)], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if "[LOGDET]" in ln]
    assert len(lines) == 1, r.stdout
    m = re.search(r"probes = (\d+), steps = (\d+), log det A = (\S+), standard error = (\S+), Ritz values in \[(\S+), (\S+)\], "
                  r"log det M = (\S+)", lines[0])
    assert m and (int(m.group(1)), int(m.group(2))) == (probes, steps), lines[0]
    assert out.read_text().startswith("%d,1," % n)
    with gpu_pkg.CGSolver(gemv_variant=-1) as s:
        s.generate_lap2d_matrix(n)
        s.set_preconditioner("pivchol", rank=16)
        want = s.logdet_pc(probes=probes, steps=steps, seed=1)
    assert float(m.group(3)) == pytest.approx(want["estimate"], rel=1e-11)         # printed with 12 digits
    assert float(m.group(4)) == pytest.approx(want["std_error"], rel=1e-5)         # ... and 6
    assert float(m.group(5)) == pytest.approx(want["ritz_min"], rel=1e-5) and float(m.group(6)) == pytest.approx(want["ritz_max"], rel=1e-5)
    assert float(m.group(7)) == pytest.approx(want["logdet_precond"], rel=1e-11)
