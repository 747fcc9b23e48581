"""cgx_solve_shifted (csrc/cgx_shift.hip, csrc/cgx_shift_host.cpp) on the MI355X: multi-shift CG, (A + sigma I) x = b for up to
16 shifts from one Krylov sequence.

- every shift against oracle.solve of the shifted dense matrix (fixed iterations and converged), dense, symmetric K1 and CSR;
- what every shift reports (both residuals, x_norm, rel_residual) against the oracle and a host recomputation, dense and CSR;
- sigma = 0 against cgx_solve on the same context, bit for bit;
- independence of the other shifts, their number, their order and check_every;
- the underflow guard of zeta, the early end when every shift is frozen;
- no interference with the single and the multi path; refusals; the fault walk over every HIP call of a shifted solve; the CLI.
"""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x3D1F
ERR_BAD_ARG, ERR_HIP, ERR_UNSUPPORTED = 1, 3, 7   # cgx_status (include/cgx.h)
S7 = [0.0, 1e-3, 0.05, 1.0, 7.5, 100.0, 1e4]
KEYS = ("iterations", "converged", "residual_prev", "residual_last", "x_norm", "rel_residual")


def _diag(n):
    return 1.03 * 2.0 * np.sqrt(n / 3.0)   # dominant diagonal: the hash matrix is SPD (tests/test_gpu_multi_rhs.py)


_cache = {}


def _problem(oracle, kind, n):
    """(A, b) of a test problem, made once: lap2d with the source term, the symmetric hash matrix with cos(i)."""
    key = ("problem", kind, n)
    if key not in _cache:
        if kind == "hash":
            _cache[key] = (oracle.hash_rows(n, 0, n, SEED, True, _diag(n)), np.cos(np.arange(n, dtype=np.float64)))
        else:
            _cache[key] = (oracle.generate_lap2d(n), oracle.init_source_term(n))
        for a in _cache[key]:
            a.setflags(write=False)
    return _cache[key]


def _reference(oracle, kind, n, sigma, max_iter, tol):
    """oracle.solve(A + sigma I, b) of a test problem, computed once and shared."""
    key = ("ref", kind, n, sigma, max_iter, tol)
    if key not in _cache:
        A, b = _problem(oracle, kind, n)
        As = A + sigma * np.eye(n)
        x, r = oracle.solve(As, b, max_iter=max_iter, tol=tol)
        x.setflags(write=False)
        _cache[key] = (x, r)
    return _cache[key]


def _solver(pkg, kind, n, storage="dense", **kw):
    fmt = pkg.MATRIX_CSR if storage == "csr" else pkg.MATRIX_DENSE
    s = pkg.CGSolver(gemv_variant=kw.pop("gemv_variant", -1), matrix_format=fmt, **kw)
    s.generate_lap2d_matrix(n)
    if kind == "hash":
        s.probe_fill_matrix_hash(SEED, symmetric=True, diag=_diag(n))
        s.set_source_term(np.cos(np.arange(n, dtype=np.float64)))
    else:
        s.init_source_term(1.0 / n)
    return s


def _tuples(res):
    return [tuple(r[k] for k in KEYS) for r in res]


# ---- 1. fixed iterations against the oracle on the shifted matrix -------------------------------------------------------------------
@pytest.mark.parametrize("kind,n,storage,variant", [("lap2d", 64, "dense", -1), ("lap2d", 257, "dense", -1), ("lap2d", 511, "dense", -1),
                                                    ("lap2d", 1000, "dense", -1), ("hash", 513, "dense", -1),
                                                    ("lap2d", 1000, "csr", -1), ("lap2d", 1000, "csr", 70008)])
def test_fixed_iterations_against_oracle(gpu_pkg, oracle, kind, n, storage, variant):
    iters = 12
    with _solver(gpu_pkg, kind, n, storage, gemv_variant=variant) as s:
        s.set_max_iter(iters)
        s.tolerance(0.0)
        X, res = s.solve_shifted(S7)
    assert X.shape == (len(S7), n)
    for j, sigma in enumerate(S7):
        xo, ro = _reference(oracle, kind, n, sigma, iters, 0.0)
        err = np.linalg.norm(X[j] - xo) / np.linalg.norm(xo)
        print("fixed %s n=%d %s sigma=%g: iterations %d, |dx|/|x| = %.2e" % (kind, n, storage, sigma, res[j]["iterations"], err))
        assert res[j]["iterations"] == ro["iterations"] == iters, (sigma, res[j], ro)
        assert err <= 1e-12, (sigma, err)


@pytest.mark.parametrize("storage", ["dense", "csr"])
def test_reported_numbers_against_oracle(gpu_pkg, oracle, storage):
    """What a shift reports, against values computed outside the library (for sigma != 0 they come from k_column_norms and the
    |zeta| sqrt(r.r) stores alone): residual_prev and residual_last against the oracle's on the shifted matrix, 1e-9 relative
    (the bar of tests/test_gpu_parity.py test_full_size_properties for reported residuals); x_norm against ||x||, 1e-12;
    rel_residual against ||(A + sigma I) x - b|| / ||b|| recomputed on the host from the returned x, 1e-9 relative plus the
    rounding allowance of tests/test_gpu_jacobi_scaled.py _check_rel_residual at 6 entries per row."""
    from test_gpu_jacobi_scaled import _check_rel_residual
    n, iters = 1000, 12
    A, b = _problem(oracle, "lap2d", n)
    with _solver(gpu_pkg, "lap2d", n, storage) as s:
        assert (s.gemv_plan()["variant"] == 7) == (storage == "csr"), s.gemv_plan()
        s.set_max_iter(iters)
        s.tolerance(0.0)
        X, res = s.solve_shifted(S7)
    for j, sigma in enumerate(S7):
        _, ro = _reference(oracle, "lap2d", n, sigma, iters, 0.0)
        xn = float(np.linalg.norm(X[j]))
        offs = {k: abs(res[j][k] - ro[k]) / ro[k] for k in ("residual_prev", "residual_last")}
        print("reported %s sigma=%g: residual_prev off by %.2e, residual_last by %.2e, x_norm by %.2e" % (
            storage, sigma, offs["residual_prev"], offs["residual_last"], abs(res[j]["x_norm"] - xn) / xn))
        assert res[j]["iterations"] == ro["iterations"] == iters, (sigma, res[j], ro)
        for k, off in offs.items():
            assert off <= 1e-9, (sigma, k, res[j][k], ro[k])
        assert abs(res[j]["x_norm"] - xn) <= 1e-12 * xn, (sigma, res[j]["x_norm"], xn)
        _check_rel_residual(res[j], A @ X[j] + sigma * X[j], np.abs(A) @ np.abs(X[j]) + sigma * np.abs(X[j]), b, 6, (storage, sigma))


# ---- 2. converged ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n", [("lap2d", 64), ("lap2d", 1000), ("hash", 513)])
def test_converged_against_oracle(gpu_pkg, oracle, kind, n):
    tol = 1e-10
    with _solver(gpu_pkg, kind, n) as s:
        s.set_max_iter(n)
        s.tolerance(tol)
        X, res = s.solve_shifted(S7)
    for j, sigma in enumerate(S7):
        xo, ro = _reference(oracle, kind, n, sigma, n, tol)
        print("converged %s n=%d sigma=%g: iterations %d (oracle %d), rel_residual %.3e (oracle %.3e)" % (
            kind, n, sigma, res[j]["iterations"], ro["iterations"], res[j]["rel_residual"], ro["rel_residual"]))
        assert res[j]["converged"] == 1, (sigma, res[j])
        assert abs(res[j]["iterations"] - ro["iterations"]) <= 0.15 * ro["iterations"] + 1, (sigma, res[j], ro)
        assert res[j]["rel_residual"] <= max(1e-11, 4.0 * ro["rel_residual"]), (sigma, res[j], ro)
    it = {sigma: res[j]["iterations"] for j, sigma in enumerate(S7)}
    assert it[1e4] < it[1.0] < it[0.0], it   # larger shifts finish strictly earlier


# ---- 3. sigma = 0 is the seed, bit for bit ----------------------------------------------------------------------------------------------
def _zero_shift_is_plain_solve(s, n):
    x = np.zeros(n)
    r = s.solve(x)
    X, res = s.solve_shifted([0.0, 3.0])
    assert np.array_equal(X[0], x)
    assert res[0]["iterations"] == r["iterations"] and res[0]["converged"] == r["converged"], (res[0], r)
    assert res[0]["residual_prev"] == r["residual_prev"], (res[0], r)
    return r, res


def test_zero_shift_bitwise_dense(gpu_pkg):
    n = 1000
    with _solver(gpu_pkg, "lap2d", n) as s:
        s.set_max_iter(40)
        s.tolerance(0.0)
        r, res = _zero_shift_is_plain_solve(s, n)
        assert r["iterations"] == 40
        s.set_max_iter(n)   # and converged: the seed's own break
        s.tolerance(1e-10)
        r, res = _zero_shift_is_plain_solve(s, n)
        assert r["converged"] == 1 and res[0]["residual_last"] == r["residual_last"]


def test_zero_shift_bitwise_csr(gpu_pkg):
    n = 1000
    with _solver(gpu_pkg, "lap2d", n, "csr") as s:
        r, res = _zero_shift_is_plain_solve(s, n)
        assert r["converged"] == 1


def test_zero_shift_bitwise_symmetric_k1(gpu_pkg):
    n = 16640   # the smallest n that takes the symmetric K1: its partial count and tail differ
    with _solver(gpu_pkg, "hash", n, gemv_variant=0) as s:
        plan = s.gemv_plan()
        assert plan["variant"] == 6, plan
        s.set_max_iter(3)
        s.tolerance(0.0)
        _zero_shift_is_plain_solve(s, n)
        assert s.gemv_plan() == plan


# ---- 4. independence --------------------------------------------------------------------------------------------------------------------
def test_permutation_and_companions_bitwise(gpu_pkg):
    n = 1000
    perm = np.random.default_rng(1).permutation(len(S7))
    others = [0.0, 0.5, 2.0, 3.0, 4.0, 5.0, 6.0, 8.0, 9.0, 10.0, 20.0, 50.0, 200.0, 1e3, 1e5]   # 15 other shifts
    with _solver(gpu_pkg, "lap2d", n) as s:
        X, res = s.solve_shifted(S7)
        Xp, resp = s.solve_shifted([S7[p] for p in perm])
        X1, res1 = s.solve_shifted([1.0])
        X16, res16 = s.solve_shifted(others[:7] + [1.0] + others[7:])
    assert np.array_equal(Xp, X[perm])
    assert _tuples(resp) == [_tuples(res)[p] for p in perm]
    j = S7.index(1.0)
    assert np.array_equal(X1[0], X[j]) and np.array_equal(X16[7], X[j])
    assert _tuples(res1)[0] == _tuples(res)[j] == _tuples(res16)[7]


def test_check_every_changes_nothing(gpu_pkg):
    n = 1000
    outs = []
    for every in (1, 16, 64):
        with _solver(gpu_pkg, "lap2d", n, check_every=every) as s:
            X, res = s.solve_shifted(S7)
            outs.append((X, _tuples(res)))
    for X, t in outs[1:]:
        assert np.array_equal(X, outs[0][0]) and t == outs[0][1]


# ---- 5. the underflow guard ------------------------------------------------------------------------------------------------------------
def test_underflow_guard(gpu_pkg, oracle):
    n, iters = 1000, 120
    A, b = _problem(oracle, "lap2d", n)
    shifts = [0.0, 300.0, 1e4]
    with _solver(gpu_pkg, "lap2d", n) as s:
        s.set_max_iter(iters)
        s.tolerance(0.0)
        x = np.zeros(n)
        r = s.solve(x)
        X, res = s.solve_shifted(shifts)
    assert np.isfinite(X).all()
    assert all(np.isfinite(res[j][k]) for j in range(3) for k in KEYS), res
    for j in (1, 2):   # zeta fell below 2^-500: frozen as converged, long after the solution stopped moving
        xe = np.linalg.solve(A + shifts[j] * np.eye(n), b)
        err = np.linalg.norm(X[j] - xe) / np.linalg.norm(xe)
        print("guard sigma=%g: frozen at %d, |dx|/|x| = %.2e" % (shifts[j], res[j]["iterations"], err))
        assert err <= 1e-12, (shifts[j], err)
        assert res[j]["converged"] == 1 and res[j]["iterations"] < iters, res[j]
    assert np.array_equal(X[0], x)
    assert res[0]["iterations"] == r["iterations"] == iters and res[0]["residual_prev"] == r["residual_prev"]


# ---- 6. the loop ends when every shift is frozen ----------------------------------------------------------------------------------------
def test_early_end_when_all_frozen(gpu_pkg):
    n = 1000
    with _solver(gpu_pkg, "lap2d", n, profile_gemv=1, check_every=4) as s:
        x = np.zeros(n)
        r = s.solve(x)
        X, res = s.solve_shifted([100.0, 1e4])
    assert r["converged"] == 1 and r["iterations"] > 100, r          # the seed alone needs about 175 iterations
    assert all(q["converged"] == 1 and q["iterations"] < 20 for q in res), res
    # every K1 launch but the first is event-timed: the host enqueued at most two polls' worth beyond the last freeze
    launches = res[0]["gemv_launches"] + res[0]["gemv_discarded"]
    print("early end: shifts frozen at %s, %d K1 launches, seed alone %d iterations" % ([q["iterations"] for q in res], launches,
                                                                                        r["iterations"]))
    assert max(q["iterations"] for q in res) < launches <= 20 + 3 * 4, (launches, res)


# ---- 7. no interference with the single and the multi path ------------------------------------------------------------------------------
@pytest.mark.parametrize("resident", [True, False])
def test_single_shifted_single(gpu_pkg, monkeypatch, resident):
    n = 2048
    if resident:
        monkeypatch.delenv("CGX_RESIDENT", raising=False)
    B = np.array([np.cos(np.arange(n) * 0.5), np.sin(np.arange(n) * 0.25) + 1.0])
    with gpu_pkg.CGSolver(gemv_variant=0 if resident else -1) as s:
        s.generate_lap2d_matrix(n)
        s.init_source_term(1.0 / n)
        s.set_max_iter(200)
        plan = s.gemv_plan()
        assert (plan["variant"] == 4) == resident, plan
        x1 = np.zeros(n)
        r1 = s.solve(x1)
        Xm1, rm1 = s.solve_multi(B)
        X, res = s.solve_shifted([0.0, 1.0, 50.0])
        assert s.gemv_plan() == plan
        x2 = np.zeros(n)
        r2 = s.solve(x2)
        Xm2, rm2 = s.solve_multi(B)
        assert s.gemv_plan() == plan
    assert np.array_equal(x1, x2)
    for key in KEYS:
        assert r1[key] == r2[key], key
    assert np.array_equal(Xm1, Xm2) and _tuples(rm1) == _tuples(rm2)
    assert np.isfinite(X).all() and res[2]["converged"] == 1 and res[2]["iterations"] < 30, res
    if not resident:   # the plain solve ran on the per-launch path too: sigma = 0 is that solve
        assert np.array_equal(X[0], x1) and res[0]["iterations"] == r1["iterations"]
        return
    # Under a persistent plan the shifted solve runs the shard's own per-launch K1 and K3, and gemv_variant 0 and -1 choose that
    # per-launch shape alike: the same kernels on the same data, so the same bits as on a context that never had a persistent
    # plan (a wrong partial count or tail offset, or a state block the persistent kernel left behind, would show here).
    with _solver(gpu_pkg, "lap2d", n) as s:
        s.set_max_iter(200)
        Xr, resr = s.solve_shifted([0.0, 1.0, 50.0])
    assert np.array_equal(X, Xr)
    assert _tuples(res) == _tuples(resr)


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------------
def _refused(s, cgx, status, shifts=(0.0, 1.0)):
    with pytest.raises(cgx.CgxError) as e:
        s.solve_shifted(list(shifts))
    assert e.value.status == status, e.value
    return str(e.value)


def test_refusals(gpu_pkg, monkeypatch):
    cgx = gpu_pkg.cgx
    n = 256
    with gpu_pkg.CGSolver(comm_mode=cgx.COMM_LOOPBACK, nranks=2, gemv_variant=-1) as s:
        s.generate_lap2d_matrix(n)
        s.init_source_term(1.0 / n)
        _refused(s, cgx, ERR_UNSUPPORTED)
        assert s.solve(np.zeros(n))["converged"] == 1   # the context is still good for what it was made for
    with gpu_pkg.CGSolver(matrix_format=cgx.MATRIX_BANDED, gemv_variant=-1) as s:
        s.generate_lap2d_matrix(n)
        s.init_source_term(1.0 / n)
        _refused(s, cgx, ERR_UNSUPPORTED)
        assert s.solve(np.zeros(n))["converged"] == 1
    monkeypatch.delenv("CGX_RESIDENT", raising=False)
    for variant in (40000, 50000):
        with gpu_pkg.CGSolver(gemv_variant=variant) as s:
            s.generate_lap2d_matrix(1024)
            s.init_source_term(1.0 / 1024)
            _refused(s, cgx, ERR_UNSUPPORTED)
            x = np.zeros(1024)
            assert s.solve(x)["converged"] == 1   # the context is still good for what it was made for
    with gpu_pkg.CGSolver(gemv_variant=-1) as s:
        s.generate_lap2d_matrix(n)
        _refused(s, cgx, ERR_BAD_ARG)                       # no source term yet
        s.init_source_term(1.0 / n)
        s.set_preconditioner("jacobi")
        _refused(s, cgx, ERR_UNSUPPORTED)
        s.set_preconditioner(None)
        X, res = s.solve_shifted([0.0, 1.0])
        assert all(r["converged"] for r in res)
        _refused(s, cgx, ERR_BAD_ARG, shifts=())
        _refused(s, cgx, ERR_BAD_ARG, shifts=[1.0] * 17)
        assert "shift 2" in _refused(s, cgx, ERR_BAD_ARG, shifts=[0.0, 1.0, -1.0])
        assert "shift 1" in _refused(s, cgx, ERR_BAD_ARG, shifts=[0.0, float("nan")])
        _refused(s, cgx, ERR_BAD_ARG, shifts=[float("inf")])
        sig = np.array([0.0, 1.0])
        Xs = np.zeros((2, n))
        L = cgx.lib()
        assert L.cgx_solve_shifted(s._h, 2, cgx._dp(sig), cgx._dp(Xs), n - 1, None) == ERR_BAD_ARG
        assert L.cgx_solve_shifted(s._h, 2, None, cgx._dp(Xs), n, None) == ERR_BAD_ARG
        assert L.cgx_solve_shifted(s._h, 2, cgx._dp(sig), None, n, None) == ERR_BAD_ARG
        s.solve_begin(np.zeros(n))
        _refused(s, cgx, ERR_BAD_ARG)                       # an open begin / end pair
        s.solve_end()
        X2, res2 = s.solve_shifted([0.0, 1.0])              # after every refusal a valid call succeeds, with the same bits
        assert np.array_equal(X2, X) and _tuples(res2) == _tuples(res)
        assert L.cgx_solve_shifted(s._h, 2, cgx._dp(sig), cgx._dp(Xs), n, None) == 0   # res may be NULL
        assert np.array_equal(Xs, X)


# ---- 9. fault walk ------------------------------------------------------------------------------------------------------------------
def test_fault_walk(gpu_pkg):
    import torch
    cgx = gpu_pkg.cgx
    n = 600
    shifts = [0.0, 2.0, 500.0]
    with _solver(gpu_pkg, "lap2d", n) as s:
        s.set_max_iter(40)
        X_ref, res_ref = s.solve_shifted(shifts)
        free0 = torch.cuda.mem_get_info()[0]
        calls = 0
        while True:
            s._set_fault_after(calls)
            try:
                X, res = s.solve_shifted(shifts)
            except cgx.CgxError as e:
                assert e.status == ERR_HIP, (calls, e)
                assert torch.cuda.mem_get_info()[0] == free0, calls
                calls += 1
                assert calls < 500
                continue
            s._set_fault_after(-1)
            break
        assert calls > 10
        X2, res2 = s.solve_shifted(shifts)
    assert np.array_equal(X2, X_ref) and np.array_equal(X, X_ref)
    assert _tuples(res2) == _tuples(res_ref) == _tuples(res)


# ---- 10. the command line ---------------------------------------------------------------------------------------------------------------
def test_cli_shifts(gpu_pkg, tmp_path):
    exe = os.path.join(ROOT, "conjugate-gradient_amd", "cgsolver")
    out = tmp_path / "out.csv"
    r = subprocess.run([exe, "1024", str(out), "--shifts", "0,1,100"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr)
    lines = [ln for ln in r.stdout.splitlines() if "[SHIFT" in ln]
    assert len(lines) == 3, r.stdout
    its = [int(ln.split("iterations = ")[1].split(",")[0]) for ln in lines]
    assert its[0] > its[1] > its[2] > 0, lines
    assert all("converged = 1" in ln for ln in lines), lines
    assert out.read_text().startswith("1024,1,")
    r = subprocess.run([exe, "1024", str(out), "--shifts", "0,1", "--jacobi"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "preconditioner" in r.stderr, (r.stdout, r.stderr)
