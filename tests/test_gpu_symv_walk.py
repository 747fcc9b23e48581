"""The walk of the symmetric K1 (plan variant 6, csrc/cgx_symv.hip): the default grid (plan_symv, kSymvRun tiles per workgroup)
against gemv_variant 60000, the same kernel on the grid of 4 workgroups per CU.

The tile kernel takes its run of tiles from gridDim.x; per-tile arithmetic, slots, fold and K3 do not depend on which workgroup
handles a tile, so the two must agree in every bit: fused solves (plain and Jacobi), the plain product and its p.Ap.
n = 16385 (nb = 65, a one-row edge tile) and 20001 (odd, a ragged edge) are the smallest sizes that select variant 6.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 0x5EEDC0DE
B = 256        # tile edge (cgx_kernels.h kSymvTile)
RUN = 1        # tiles per workgroup of the default walk (cgx_kernels.h kSymvRun)
GRID_WALK = 60000
SIZES = [16385, 20001]


def _diag(n):
    return 1.03 * 2.0 * np.sqrt(n / 3.0)   # SPD hash matrix (tests/test_gpu_symmetric.py)


@pytest.fixture(autouse=True)
def _no_walk_override(monkeypatch):
    monkeypatch.delenv("CGX_SYMV_RUN", raising=False)
    monkeypatch.delenv("CGX_GEMV_VARIANT", raising=False)


def _solve_in_pieces(pkg, n, variant, jacobi, seed=SEED):
    with pkg.CGSolver(gemv_variant=variant) as s:
        s.generate_lap2d_matrix(n)
        s.probe_fill_matrix_hash(seed, symmetric=True, diag=_diag(n))
        assert s.gemv_plan()["variant"] == 6
        if jacobi:
            s.set_preconditioner("jacobi")
        s.init_source_term(1.0 / n)
        s.set_max_iter(n)
        s.tolerance(0.0)
        s.solve_begin(np.zeros(n))
        for steps in (1, 5, 31):
            assert not s.solve_steps(steps)
        x = np.zeros(n)
        res = s.solve_end(x)
    return x, res


@pytest.mark.parametrize("jacobi", [False, True], ids=["plain", "jacobi"])
@pytest.mark.parametrize("n", SIZES)
def test_fused_solves_agree_bit_for_bit(gpu_pkg, n, jacobi):
    x0, r0 = _solve_in_pieces(gpu_pkg, n, -1, jacobi)
    x1, r1 = _solve_in_pieces(gpu_pkg, n, GRID_WALK, jacobi)
    assert r0["iterations"] == r1["iterations"] == 37
    assert np.all(np.isfinite(x0)) and np.any(x0 != 0.0)
    assert np.array_equal(x0, x1)
    assert r0["residual_prev"] == r1["residual_prev"]


@pytest.mark.parametrize("n", SIZES)
def test_plain_product_and_plan(gpu_pkg, n):
    import torch

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    nb = (n + B - 1) // B
    tiles = nb * (nb + 1) // 2
    pv = np.random.default_rng(n).standard_normal(n)
    out = {}
    for variant in (-1, GRID_WALK):
        with gpu_pkg.CGSolver(gemv_variant=variant) as s:
            s.generate_lap2d_matrix(n)
            s.probe_fill_matrix_hash(SEED + n, symmetric=True)
            out[variant] = (s.gemv_plan(), *s.probe_gemv(pv))
    (p0, y0, pap0), (p1, y1, pap1) = out[-1], out[GRID_WALK]
    assert p0["variant"] == 6 and p1["variant"] == 6, (p0, p1)
    assert p0["grid"] == max(1, tiles // RUN) and p0["U"] == -(-tiles // p0["grid"]), p0
    assert p1["grid"] == min(tiles, 4 * cus) and p1["U"] == -(-tiles // p1["grid"]), p1
    for k in ("R", "waves", "light", "split", "ncols"):
        assert p0[k] == p1[k], (k, p0, p1)
    assert np.all(np.isfinite(y0)) and np.any(y0 != 0.0)
    assert np.array_equal(y0, y1)
    assert pap0 == pap1


def test_grid_walk_code_runs_the_default_general_kernel_on_an_asymmetric_matrix(gpu_pkg):
    n = 16385
    plans = []
    for variant in (-1, GRID_WALK):
        with gpu_pkg.CGSolver(gemv_variant=variant) as s:
            s.generate_lap2d_matrix(n)
            s.probe_fill_matrix_hash(SEED, symmetric=False)
            plans.append(s.gemv_plan())
    assert plans[0]["variant"] == 1 and plans[0] == plans[1], plans
