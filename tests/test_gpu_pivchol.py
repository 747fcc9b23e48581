"""GPU tests of the pivoted-Cholesky low-rank preconditioner (include/cgx.h CGX_PRECOND_PIVCHOL) on dense
kernel matrices A = S K S + sigma^2 I built here with numpy (tests/pivchol_reference.py): the factor the device makes, the
Woodbury apply through the loop's kernels, whole solves against numpy PCG in fp64 and longdouble with the device's own L and
delta, independence of check_every and of earlier problems, staleness, the K1 forms, the refusals, the error paths and the CLI.
Every reference number is computed here; none is hard-coded."""
import os
import subprocess

import numpy as np
import pytest

import pivchol_reference as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG, ERR_HIP, UNSUPPORTED = 1, 3, 7
ELL, SIGMA2 = 0.2, 1e-2
SHAPES = [(1024, 1), (1024, 5), (1024, 64), (1024, 100), (1024, 256), (1000, 64), (1101, 64)]   # the odd sizes: a ragged last tile
_CACHE = {}


def _problem(n):
    return ref.kernel_matrix(n, ELL, SIGMA2)


def _solver(gpu_pkg, n, variant=-1, **kw):
    A, b = _problem(n)
    s = gpu_pkg.CGSolver(gemv_variant=variant, **kw)
    s.set_matrix_dense(A)
    s.set_source_term(b)
    s.set_max_iter(3000)
    s.tolerance(1e-6 * float(np.linalg.norm(b)))
    return s


def _vectors(n):
    _, b = _problem(n)
    e7 = np.zeros(n)
    e7[7] = 1.0
    return {"b": np.array(b), "e_7": e7, "random": np.random.default_rng(7).standard_normal(n)}


def _device_factor(gpu_pkg, n, rank, check=None, **kw):
    """What the device made for (n, rank), once per session: pivots, L, delta, P^-1 of three vectors, delta with shift 0.25.
    kw: further settings of the context (a row pitch, say), part of the key; check(s): asserted on the context first."""
    key = (n, rank) + tuple(sorted(kw.items()))
    if key not in _CACHE:
        with _solver(gpu_pkg, n, **kw) as s:
            if check is not None:
                check(s)
            s.set_preconditioner("pivchol", rank=rank)
            assert s.preconditioner == "pivchol" and s.preconditioner_rank() == rank
            assert s.preconditioner_shift() == (0.0, 0.0)          # nothing made yet
            s.solve_begin(np.zeros(n))
            piv, L, delta = s._probe_precond_lowrank()
            assert s.preconditioner_shift() == (0.0, delta)
            z = {k: s._probe_precond_apply(v) for k, v in _vectors(n).items()}
            s.solve_end(None)
            s.set_preconditioner("pivchol", rank=rank, shift=0.25)
            s.solve_begin(np.zeros(n))
            fixed = s.preconditioner_shift()
            s.solve_end(None)
        _CACHE[key] = {"piv": piv, "L": L, "delta": delta, "z": z, "fixed": fixed}
    return _CACHE[key]


# ---- 1. the factor -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,rank", SHAPES)
def test_factor(gpu_pkg, n, rank):
    _check_factor(_device_factor(gpu_pkg, n, rank), n, rank)


def _check_factor(f, n, rank):
    A, _ = _problem(n)
    piv, L, delta = f["piv"], f["L"], f["delta"]
    assert len(set(piv.tolist())) == rank and piv.min() >= 0 and piv.max() < n
    ratio, mean_ld = ref.remaining_diagonal_checks(A, piv, L)
    err = ref.pivot_row_error(A, piv, L)
    bar = 8 * rank * ref.EPS * np.abs(A).max()
    print("n=%d rank=%d: smallest pivot ratio %.17g, pivot rows |A - L L^T| %.3e (bar %.3e), delta %.17g" % (n, rank, ratio, err, bar, delta))
    assert ratio >= 1.0 - 1e-9
    assert err <= bar
    for t in range(rank):
        assert np.all(L[piv[:t], t] == 0.0), t                     # exactly 0 at the rows chosen earlier
        assert L[piv[t], t] > 0.0
    assert abs(ref.LD(delta) - mean_ld) <= 1e-8 * mean_ld
    assert f["fixed"] == (0.25, 0.25)


# ---- 2. the apply --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,rank", SHAPES)
def test_apply(gpu_pkg, n, rank):
    _check_apply(_device_factor(gpu_pkg, n, rank), n, rank)


def _check_apply(f, n, rank):
    w64 = ref.Woodbury(f["L"], f["delta"], np.float64)
    wld = ref.Woodbury(f["L"], f["delta"], ref.LD)
    for name, v in _vectors(n).items():
        z_ld = wld.apply(v)
        z_64 = w64.apply(v)
        zmax = float(np.abs(z_ld).max())
        bar = 100.0 * max(float(np.abs(z_64 - z_ld).max()), ref.EPS * zmax)
        got = float(np.abs(f["z"][name] - z_ld).max())
        print("n=%d rank=%d %s: |z_gpu - z_ld|_inf = %.3e, numpy fp64 %.3e, bar %.3e, ratio to bar %.3f" % (
            n, rank, name, got, float(np.abs(z_64 - z_ld).max()), bar, got / bar))
        assert got <= bar, (name, got, bar)


# ---- 3. the solve --------------------------------------------------------------------------------------------------------------
def _plain_iterations(gpu_pkg, n):
    if ("plain", n) not in _CACHE:
        with _solver(gpu_pkg, n) as s:
            res = s.solve(np.zeros(n))
        assert res["converged"] == 1
        _CACHE[("plain", n)] = res["iterations"]
    return _CACHE[("plain", n)]


def _references(n, L, delta, tol):
    A, b = _problem(n)
    r64 = ref.pcg(A, b, ref.Woodbury(L, delta, np.float64).apply, tol, 400, np.float64)
    rld = ref.pcg(A, b, ref.Woodbury(L, delta, ref.LD).apply, tol, 400, ref.LD)
    k = rld["iterations"]
    # a case is usable only where the stop is not a matter of rounding: both references stop at k, clearly below tol there and
    # clearly above it one step earlier
    assert r64["iterations"] == k and r64["converged"] == rld["converged"] == 1
    for r in (r64, rld):
        assert r["hist"][k + 1] <= 0.95 * tol and r["hist"][k] >= 1.05 * tol, (r["hist"][k + 1] / tol, r["hist"][k] / tol)
    return r64, rld


def _check_solve(x, res, n, L, delta):
    _, b = _problem(n)
    bn = float(np.linalg.norm(b))
    tol = 1e-6 * bn
    r64, rld = _references(n, L, delta, tol)
    k = rld["iterations"]
    dist = float(np.linalg.norm(r64["x"] - rld["x"]) / np.linalg.norm(rld["x"]))
    got = float(np.linalg.norm(x - rld["x"]) / np.linalg.norm(rld["x"]))
    print("k=%d (stop at %.3f tol, %.3f tol one step earlier), |x - x_ld|/|x| = %.3e, numpy fp64 %.3e, rel_residual %.3e" % (
        k, rld["hist"][k + 1] / tol, rld["hist"][k] / tol, got, dist, res["rel_residual"]))
    assert res["iterations"] == k and res["converged"] == 1
    assert res["rel_residual"] <= 10 * tol / bn
    assert got <= max(100 * dist, 1e-12)
    return k


@pytest.mark.parametrize("rank", [64, 128])
def test_solve(gpu_pkg, rank):
    n = 1024
    with _solver(gpu_pkg, n) as s:
        s.set_preconditioner("pivchol", rank=rank)
        x = np.zeros(n)
        res = s.solve(x)
        _, L, delta = s._probe_precond_lowrank()
    k = _check_solve(x, res, n, L, delta)
    plain = _plain_iterations(gpu_pkg, n)
    print("rank %d: %d iterations against %d of plain CG" % (rank, k, plain))
    assert 4 * res["iterations"] <= plain


# ---- 4. independence and staleness ---------------------------------------------------------------------------------------------
def _bits(a, b):
    (xa, ra), (xb, rb) = a, b
    assert np.array_equal(xa, xb)
    for key in ("iterations", "converged", "residual_prev", "residual_last", "x_norm", "rel_residual"):
        assert ra[key] == rb[key], key


def _run(s, n):
    x = np.zeros(n)
    return x, s.solve(x)


def test_repeats_and_check_every(gpu_pkg):
    n = 1024
    with _solver(gpu_pkg, n, check_every=1) as s:
        s.set_preconditioner("pivchol", rank=64)
        a = _run(s, n)
        _bits(_run(s, n), a)
    with _solver(gpu_pkg, n, check_every=16) as s:
        s.set_preconditioner("pivchol", rank=64)
        _bits(_run(s, n), a)


def test_second_matrix_matches_a_fresh_context(gpu_pkg):
    n, n2 = 1024, 1000
    A2, b2 = _problem(n2)
    with _solver(gpu_pkg, n) as s:
        s.set_preconditioner("pivchol", rank=64)
        _run(s, n)
        s.set_matrix_dense(A2)
        s.set_source_term(b2)
        s.set_max_iter(3000)
        assert s.preconditioner == "pivchol" and s.preconditioner_rank() == 64   # the settings survive a new matrix
        assert s.preconditioner_shift() == (0.0, 0.0)                            # ... the factor does not
        second = _run(s, n2)
    with _solver(gpu_pkg, n2) as s:
        s.tolerance(1e-6 * float(np.linalg.norm(_problem(n)[1])))                # (the first context's tolerance)
        s.set_preconditioner("pivchol", rank=64)
        _bits(_run(s, n2), second)


def test_rank_and_shift_remake_the_factor(gpu_pkg):
    n = 1024
    with _solver(gpu_pkg, n) as s:
        s.set_preconditioner("pivchol", rank=32)
        _run(s, n)
        _, L32, d32 = s._probe_precond_lowrank()
        s.set_preconditioner("pivchol", rank=48)
        with pytest.raises(gpu_pkg.CgxError) as e:                               # stale until the next begin
            s._probe_precond_lowrank()
        assert e.value.status == BAD_ARG
        _run(s, n)
        _, L48, d48 = s._probe_precond_lowrank()
        assert L48.shape == (n, 48) and np.array_equal(L48[:, :32], L32) and np.any(L48[:, 32:] != 0.0) and d48 < d32
        s.set_preconditioner("pivchol", rank=48, shift=2.0 * d48)
        r_shift = _run(s, n)
        _, L48b, d48b = s._probe_precond_lowrank()
        assert d48b == 2.0 * d48 and np.array_equal(L48b, L48)
        z1 = s._probe_precond_apply(np.ones(n))
        s.set_preconditioner("pivchol", rank=48)
        r_auto = _run(s, n)
        assert not np.array_equal(s._probe_precond_apply(np.ones(n)), z1)
        assert r_shift[1]["converged"] == r_auto[1]["converged"] == 1


def test_clearing_the_kind_gives_the_plain_bits_and_the_persistent_plan(gpu_pkg, monkeypatch):
    monkeypatch.delenv("CGX_RESIDENT", raising=False)
    n = 1024
    A, b = _problem(n)

    def make():
        s = gpu_pkg.CGSolver()
        s.set_matrix_dense(A)
        s.set_source_term(b)
        s.set_max_iter(200)
        s.tolerance(1e-6 * float(np.linalg.norm(b)))
        return s

    with make() as s:
        before = s.gemv_plan()
        assert before["variant"] == 4                                            # the LDS-resident persistent kernel
        s.set_preconditioner("pivchol", rank=64)
        assert s.gemv_plan()["variant"] == 1                                     # parked on the per-launch path
        assert _run(s, n)[1]["converged"] == 1
        s.set_preconditioner(None)
        assert s.gemv_plan() == before
        after = _run(s, n)
    with make() as s:
        _bits(_run(s, n), after)
    with _solver(gpu_pkg, n) as s:                                               # and on the per-launch path itself
        plain = _run(s, n)
        s.set_preconditioner("pivchol", rank=16)
        _run(s, n)
        s.set_preconditioner(None)
        _bits(_run(s, n), plain)


# ---- 5. the K1 forms -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [-1, 10821, 20421])   # the library's choice of the general K1 (per-launch path), an explicit shape of it, the LDS-staged K1
def test_general_k1_forms(gpu_pkg, variant):
    n = 1024
    with _solver(gpu_pkg, n, variant=variant) as s:
        s.set_preconditioner("pivchol", rank=64)
        x = np.zeros(n)
        res = s.solve(x)
        plan = s.gemv_plan()
        _, L, delta = s._probe_precond_lowrank()
    assert plan["variant"] == (2 if variant == 20421 else 1)
    _check_solve(x, res, n, L, delta)


def test_symmetric_k1(gpu_pkg):
    n, seed = 16640, 20261018
    b = np.sin(0.37 * np.arange(n)) + 0.5
    out = {}
    for variant in (0, 10821):
        with gpu_pkg.CGSolver(gemv_variant=variant) as s:
            s.generate_lap2d_matrix(n)
            s.probe_fill_matrix_hash(seed, symmetric=True, diag=9000.0)   # filled on the device: no host matrix
            s.set_source_term(b)
            s.set_max_iter(200)
            s.tolerance(1e-8 * float(np.linalg.norm(b)))
            s.set_preconditioner("pivchol", rank=16)
            out[variant] = (s.gemv_plan()["variant"],) + _run(s, n)
    assert out[0][0] == 6 and out[10821][0] == 1
    (_, x6, r6), (_, x1, r1) = out[0], out[10821]
    assert r6["converged"] == r1["converged"] == 1 and r6["iterations"] == r1["iterations"] > 0
    assert np.linalg.norm(x6 - x1) <= 1e-10 * np.linalg.norm(x1)
    assert r6["rel_residual"] <= 1e-7


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------
def _refused(gpu_pkg, s, n, status):
    with pytest.raises(gpu_pkg.CgxError) as e:
        s.solve(np.zeros(n))
    assert e.value.status == status, e.value
    return str(e.value)


def test_refusals(gpu_pkg):
    n = 1024   # (gemv_variant 50000 takes no smaller problem)
    for kw in ({"comm_mode": gpu_pkg.COMM_LOOPBACK, "nranks": 2}, {"matrix_format": gpu_pkg.MATRIX_BANDED},
               {"matrix_format": gpu_pkg.MATRIX_CSR}, {"gemv_variant": 40000}, {"gemv_variant": 50000},
               {"gemv_variant": 10825}):   # (the last: K1 leaves Ap as column pieces for a prefold kernel the loop does not run)
        with gpu_pkg.CGSolver(**kw) as s:
            s.generate_lap2d_matrix(n)
            s.init_source_term(1.0 / n)
            s.set_preconditioner("pivchol", rank=8)
            _refused(gpu_pkg, s, n, UNSUPPORTED)
    with gpu_pkg.CGSolver(gemv_variant=-1) as s:
        s.generate_lap2d_matrix(n)
        s.init_source_term(1.0 / n)
        s.set_preconditioner("pivchol", rank=8)
        with pytest.raises(gpu_pkg.CgxError) as e:
            s.solve_multi(np.ones((2, n)))
        assert e.value.status == UNSUPPORTED
        with pytest.raises(gpu_pkg.CgxError) as e:
            s.solve_shifted([0.0, 1.0])
        assert e.value.status == UNSUPPORTED
    with gpu_pkg.CGSolver(gemv_variant=-1) as s:                                 # rank > n
        s.generate_lap2d_matrix(100)
        s.init_source_term(0.01)
        s.set_preconditioner("pivchol", rank=101)
        _refused(gpu_pkg, s, 100, BAD_ARG)
        s.set_preconditioner("pivchol", rank=100, shift=1.0)                     # rank == n needs a shift of its own
        assert s.solve(np.zeros(100))["converged"] == 1


def test_a_matrix_that_is_not_positive_definite(gpu_pkg):
    n = 1024
    A, b = _problem(n)
    bad = np.array(A)
    bad[321, 321] = -1.0e6
    with gpu_pkg.CGSolver(gemv_variant=-1) as s:
        s.set_matrix_dense(bad)
        s.set_source_term(b)
        s.set_preconditioner("pivchol", rank=16)
        msg = _refused(gpu_pkg, s, n, BAD_ARG)
        assert "row 321" in msg, msg
        s.set_preconditioner(None)                                               # the context stays usable
        s.set_matrix_dense(A)
        s.set_source_term(b)
        s.set_max_iter(3000)
        s.tolerance(1e-6 * float(np.linalg.norm(b)))
        got = _run(s, n)
    with _solver(gpu_pkg, n) as s:
        _bits(_run(s, n), got)


def test_setters_are_refused_inside_a_solve(gpu_pkg):
    n = 1024
    L = gpu_pkg.cgx.lib()
    with _solver(gpu_pkg, n) as s:
        s.set_preconditioner("pivchol", rank=16)
        assert L.cgx_set_preconditioner_rank(s._h, 0) == BAD_ARG
        assert L.cgx_set_preconditioner_rank(s._h, 257) == BAD_ARG
        assert L.cgx_set_preconditioner_shift(s._h, -1.0) == BAD_ARG
        assert L.cgx_set_preconditioner_shift(s._h, float("nan")) == BAD_ARG
        assert L.cgx_set_preconditioner_shift(s._h, float("inf")) == BAD_ARG
        s.solve_begin(np.zeros(n))
        assert L.cgx_set_preconditioner_rank(s._h, 8) == BAD_ARG
        assert L.cgx_set_preconditioner_shift(s._h, 0.5) == BAD_ARG
        assert L.cgx_set_preconditioner(s._h, 0) == BAD_ARG
        s.solve_steps(3)
        s.solve_end(None)
        assert s.preconditioner_rank() == 16 and s.preconditioner_shift()[0] == 0.0
        _, L16, d16 = s._probe_precond_lowrank()
        s.set_preconditioner("jacobi")                                           # another kind leaves rank, shift and factor alone
        s.set_preconditioner(None)                                               # the probes need the kind
        assert s.preconditioner_rank() == 16 and s.preconditioner_shift() == (0.0, d16)
        with pytest.raises(gpu_pkg.CgxError) as e:
            s._probe_precond_apply(np.ones(n))
        assert e.value.status == BAD_ARG


# ---- 7. error paths ------------------------------------------------------------------------------------------------------------
def _walk(gpu_pkg, s, attempt, before=None):
    """Fail the 1st, 2nd, ... runtime call of `attempt` until it runs through; returns how many failures that took."""
    calls = 0
    while True:
        if before:
            before()
        s._set_fault_after(calls)
        try:
            attempt()
        except gpu_pkg.CgxError as e:
            assert e.status == ERR_HIP, (calls, e)
            calls += 1
            assert calls < 400
            continue
        s._set_fault_after(-1)
        return calls


def test_fault_walk_over_a_begin_and_a_steps_call(gpu_pkg):
    """Host-side injection: the (N+1)-th runtime call of the context is not made and reports an error.  Nothing faults on the
    device.  Every injected failure must surface as an error, and the context must solve correctly afterwards."""
    import torch
    n = 1000

    def finish(s):
        s.solve_steps(3000)
        x = np.zeros(n)
        return x, s.solve_end(x)

    with _solver(gpu_pkg, n) as s:
        s.set_preconditioner("pivchol", rank=16)
        ref_run = _run(s, n)
        free0 = torch.cuda.mem_get_info()[0]

        def stale():   # the factor goes stale, so every begin below makes it again (a failed begin leaves no solve open)
            s.set_preconditioner("pivchol", rank=8)
            s.set_preconditioner("pivchol", rank=16)

        calls = _walk(gpu_pkg, s, lambda: s.solve_begin(np.zeros(n)), before=stale)
        assert calls > 30, calls                                                 # 16 steps alone are 16 launches
        _bits(finish(s), ref_run)

        def begin_and_steps():   # the factor stands: the rest of the begin, and four iterations with their poll
            s.solve_begin(np.zeros(n))
            s.solve_steps(4)

        calls = _walk(gpu_pkg, s, begin_and_steps)
        assert calls > 20, calls
        _bits(finish(s), ref_run)
        _bits(_run(s, n), ref_run)
        assert torch.cuda.mem_get_info()[0] == free0                             # nothing leaked on the way


# ---- 8. the CLI ----------------------------------------------------------------------------------------------------------------
def test_cli(gpu_pkg, tmp_path):
    exe = os.path.join(ROOT, "conjugate-gradient_amd", "cgsolver")
    out = tmp_path / "out.csv"
    r = subprocess.run([exe, "256", str(out), "--pivchol", "16", "--stats"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "precond=pivchol rank=16" in r.stderr and "converged=1" in r.stderr, r.stderr
    assert "[STEP" in r.stdout and out.read_text().startswith("256,1,")
    r = subprocess.run([exe, "256", str(out), "--pivchol", "16", "--pivchol-shift", "0.5", "--stats"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0 and "shift=0.5 " in r.stderr and "converged=1" in r.stderr, r.stderr
