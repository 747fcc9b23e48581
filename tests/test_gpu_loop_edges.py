"""The edges of the polled host loop (run_polled, csrc/cgx_internal.h) on the MI355X, for the three entry points that share it:
cgx_solve (begin / steps / end), cgx_solve_multi and cgx_solve_shifted.

lap2d, n = 1024, the per-launch path (gemv_variant -1), source term 1/n, the default tolerance, check_every = 16, and iteration
limits on both sides of one batch and of two: 1, 15, 16, 17, 33.  None of the systems converges that early (the seed needs about
175 iterations at this size), so the loop always runs out at the limit:

- every solve reports iterations == max_iter and converged == 0;
- x and the result scalars do not depend on check_every (1, 16, 64), bit for bit;
- cgx_solve_steps in pieces of 5, 12 and 16 gives the bits of the single cgx_solve;
- with every K1 launch event-timed, timed + discarded launches == max_iter for all three, and the device-side window of the
  steps (steps_device_ms) is recorded by cgx_solve and cgx_solve_shifted and left at 0 by cgx_solve_multi.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 1024
LIMITS = (1, 15, 16, 17, 33)
SHIFTS = [0.0, 1.0]
KEYS = ("iterations", "converged", "residual_prev", "residual_last", "x_norm", "rel_residual")

_cache = {}


def _rhs():
    i = np.arange(N, dtype=np.float64)
    return np.array([np.cos(0.5 * i), np.sin(0.25 * i) + 1.0])


def _solver(pkg, max_iter, check_every, profile=0):
    s = pkg.CGSolver(gemv_variant=-1, check_every=check_every, profile_gemv=profile)
    s.generate_lap2d_matrix(N)
    s.init_source_term(1.0 / N)
    s.set_max_iter(max_iter)
    return s


def _tuple(r):
    return tuple(r[k] for k in KEYS)


def _three_solves(pkg, max_iter, check_every, profile=0):
    """{'solve': (x, [res]), 'multi': (X, [res, res]), 'shifted': (X, [res, res])} of one context, made once and left unchanged."""
    key = (max_iter, check_every, profile)
    if key not in _cache:
        with _solver(pkg, max_iter, check_every, profile) as s:
            x = np.zeros(N)
            r = s.solve(x)
            Xm, rm = s.solve_multi(_rhs())
            Xs, rs = s.solve_shifted(SHIFTS)
        for a in (x, Xm, Xs):
            a.setflags(write=False)
        _cache[key] = {"solve": (x, [r]), "multi": (Xm, rm), "shifted": (Xs, rs)}
    return _cache[key]


@pytest.mark.parametrize("max_iter", LIMITS)
def test_loop_runs_out_at_the_limit(gpu_pkg, max_iter):
    out = _three_solves(gpu_pkg, max_iter, 16)
    for name, (X, res) in out.items():
        print("max_iter %d %s: %s" % (max_iter, name, [(r["iterations"], r["converged"]) for r in res]))
    for name, (X, res) in out.items():
        assert np.isfinite(X).all(), name
        for r in res:
            assert r["iterations"] == max_iter and r["converged"] == 0, (name, r)


@pytest.mark.parametrize("max_iter", LIMITS)
def test_check_every_changes_nothing(gpu_pkg, max_iter):
    ref = _three_solves(gpu_pkg, max_iter, 16)
    for every in (1, 64):
        out = _three_solves(gpu_pkg, max_iter, every)
        for name in ref:
            assert np.array_equal(out[name][0], ref[name][0]), (every, name)
            assert [_tuple(r) for r in out[name][1]] == [_tuple(r) for r in ref[name][1]], (every, name)


def test_steps_in_pieces(gpu_pkg):
    max_iter = 33
    x_ref, (r_ref,) = _three_solves(gpu_pkg, max_iter, 16)["solve"]
    with _solver(gpu_pkg, max_iter, 16) as s:
        s.solve_begin(np.zeros(N))
        for piece in (5, 12, 16):
            assert s.solve_steps(piece) is False
        x = np.zeros(N)
        r = s.solve_end(x)
    assert np.array_equal(x, x_ref)
    assert _tuple(r) == _tuple(r_ref), (r, r_ref)


@pytest.mark.parametrize("max_iter", LIMITS)
def test_profiled_launch_counts_and_window(gpu_pkg, max_iter):
    out = _three_solves(gpu_pkg, max_iter, 16, profile=1)
    for name, (X, res) in out.items():
        r = res[0]
        print("max_iter %d %s: %d timed + %d discarded K1 launches, steps_device_ms %.6f" % (
            max_iter, name, r["gemv_launches"], r["gemv_discarded"], r["steps_device_ms"]))
    for name, (X, res) in out.items():
        for r in res:
            assert r["gemv_launches"] + r["gemv_discarded"] == max_iter, (name, r)
    assert out["solve"][1][0]["steps_device_ms"] > 0
    assert all(r["steps_device_ms"] > 0 for r in out["shifted"][1])
    assert all(r["steps_device_ms"] == 0.0 for r in out["multi"][1])
