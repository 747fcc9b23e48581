"""Every per-launch kernel at row pitches without pad columns (cgx_config.lda_pad = 0, or CGX_LDA_PAD=0).

The pitch of A and of every vector laid out like a row of A is lda = roundup(n, 16) + roundup(lda_pad, 2) (default_lda,
csrc/cgx_context.cpp; the default pad is 16).  With lda_pad = 0 and n % 16 == 0 the pitch equals n: A has no column behind n, no
vector an element behind n, and the columns of the multi-right-hand-side and shifted blocks, of the low-rank factor L, of block
Jacobi's W and the slots of the symmetric K1 touch.  The rest of the suite runs these kernels with 16 spare zero doubles behind
every row and vector, which would hide a read or write one element too far.  Here every kernel family runs at pad 0 (and the
general K1 at pad 2) against a high-precision reference or the oracle, and bit for bit (np.array_equal) against the default pitch.
Every test asserts the pitch it runs at first: cgx_get_matrix_format reports 8 * rows * lda for dense storage.  CSR and banded
storage do not show the pitch; there it is asserted on a dense context made with the same configuration.

Address audit at lda == n (n % 16 == 0), and lda == n + 1 ... n + 15 for the other n (lda is always even, so an odd n has at least
one pad element).  Allocations: A rows * lda; p[0], p[1], dinv lda; r lda + G (G = update_xr_grid(n) r.r partials behind it); z
lda + 2 G; Ap segment Sr = roundup(rows, 2) plus a tail; W block * lda; L rank * lda; symmetric slots nb * lda; the multi and shift
blocks 16 * lda per vector (cgx_context.cpp, cgx_precond.cpp, cgx_multi_host.cpp, cgx_shift_host.cpp, cgx_minres_host.cpp).

  kernel                    access                                  bound            why it holds
  k_gemv_colsplit           v, r, p_new, A row + c, c + 1           c + 1 < ncols    ncols = min(roundup(n, 2), lda); c is even
    one-round form          first trip ahead of the head            c + (U-1) * 512 + 1 < ncols   full(c) guards the whole trip
    one-round form          epilogue operands v[j], r[j]            j <= ncols - 1   clamped index
  k_gemv_ldsp               v, r, p_new, A row + c, c + 1           c + 1 < lda      the sweep is lda wide; c and lda are even
  k_prefold_ap              parts + sp * Sr + rc, rc + 1            rc <= Sr - 2     clamped; p_loc[row] clamped to rows - 1
  k_update_xr*, k_init_*    r[i], z[i], dinv[i], p[i], x[li]        i < n            guarded
                            r[lda + wg], z[lda + wg], z[lda+G+wg]   wg < G           the partials have their own G (2 G) doubles
  bj_issue / bj_chain       W[t * lda + i]                          t < B, i < n     rows past n are clamped to row 0
  k_bj_col_slice / _invert  W[j * lda + s + i]                      s + i < n, j < B guarded by m = min(B, n - s)
  k_lr_step / _update / _apply / _gram   L[u * lda + i]             u < rank, i < n  guarded or clamped to n - 1
  k_multi_gemv              V, R, P at j * lda + col, col + 1       col + 1 < roundup(n, 2) <= lda   live columns only
  k_multi_update / _init    j * lda + i                             i < n            guarded
  k_shift_update / _begin   X, P at j * lda + i                     i < n (begin: i < lda)   guarded, j < nshift
  k_minres_init             w, vprev at i; X, D[0], D[1] at j * lda + i   i < lda, j < nshift   the side block of cgx_minres_host.cpp: X,
                                                                                     D[0], D[1], Y 16 * lda each, two vectors of lda, end to
                                                                                     end; b[i] is read for i < n only, rows n .. lda get 0
  k_minres_step / _close    w, Y, vprev at i; X, D at j * lda + i   i < n, j < nshift   stores guarded, first-trip loads clamped to row 0
                            ww_in[wg], ww_out[wg]                   wg < G           and to shift 0; the partials have their own 2 G doubles
  k_symv_tiles              v, r, p_new at c, c + 1; A row + col    c + 1 < ncols    vec2 guards, col clamped to ncols - 2
                            parts[J * lda + i]                      i < n, J < nb    guarded
  k_symv_fold               parts[s * lda + rc], p[rc], rc + 1      rc + 1 < roundup(n, 2) <= lda   row n of an odd n lies in the
                                                                                     pad of its slot, which is never written
  k_spmv_csr                v[col], r[col], p_new[cc]               col < n, cc < lda   scalar accesses, the pre-pass count is 0
  k_spmv_dia, _dia_lds      v, r at the pair (jb, jb + 1), jb = clamp(row + off, 0, n - 1); v, r, p_new at the pair (g, g + 1)
                            NOT inside at lda == n: jb = n - 1 and (last row of the last shard, odd row count) g = n - 1 touched
                            element n -- a read behind p, and in the fused form a write.  Both kernels now load such a pair one
                            element lower and take 0 for its upper half (what a pad holds), and store p_new[n - 1] alone:
                            test_banded_* below.  The staged windows of the LDS form were guarded already (c + 1 < lda).

Pitch independence: every kernel's summation order is a function of the column index and n; k_gemv_ldsp alone sweeps the pad and
adds exact zeros there.  No exception was needed: every comparison below is bit for bit."""
import numpy as np
import pytest

import test_gpu_banded as tb
import test_gpu_block_jacobi as bj
import test_gpu_csr as tc
import test_gpu_jacobi_scaled as js
import test_gpu_minres as mn
import test_gpu_multi_rhs as mr
import test_gpu_parity as tp
import test_gpu_pivchol as pv
import test_gpu_shifted as sh
import test_gpu_symmetric_parity as sp

pytestmark = pytest.mark.gpu

DEFAULT = -1   # cgx_config.lda_pad as cgx_config_init leaves it: the environment variable, else 16
KEYS = ("iterations", "converged", "residual_prev", "residual_last", "x_norm", "rel_residual")
LD = np.longdouble


@pytest.fixture(autouse=True)
def _library_defaults(monkeypatch):
    monkeypatch.delenv("CGX_LDA_PAD", raising=False)
    monkeypatch.delenv("CGX_GEMV_VARIANT", raising=False)
    monkeypatch.delenv("CGX_SYMV_RUN", raising=False)


def n16(n):
    return (n + 15) // 16 * 16


def pitch(n, pad):
    return n16(n) + (16 if pad < 0 else (pad + 1) // 2 * 2)


def assert_pitch(s, n, pad, p=1):
    """Dense storage: every local shard holds rows x lda doubles at the pitch under test."""
    for q in range(p):
        rows = n // p if q < p - 1 else n - (n // p) * (p - 1)
        fmt, _, nbytes = s.matrix_format(q)
        assert fmt == 0 and nbytes == 8.0 * max(rows, 1) * pitch(n, pad), (n, pad, q, fmt, nbytes)


def assert_pitch_on_dense_twin(pkg, n, pad, p=1):
    """CSR and banded storage: the pitch of a dense context made with the same configuration."""
    mode = pkg.COMM_SELF if p == 1 else pkg.COMM_LOOPBACK
    with pkg.CGSolver(comm_mode=mode, nranks=p, lda_pad=pad) as s:
        s.generate_lap2d_matrix(n)
        assert_pitch(s, n, pad, p)


def same_solve(a, b, what=None):
    (xa, ra), (xb, rb) = a, b
    assert np.all(np.isfinite(xa)) and np.any(xa != 0.0), what
    assert np.array_equal(xa, xb), (what, int(np.count_nonzero(xa != xb)))
    for key in KEYS:
        assert ra[key] == rb[key], (what, key, ra[key], rb[key])


def _shards(pkg, p):
    return dict(comm_mode=pkg.COMM_SELF if p == 1 else pkg.COMM_LOOPBACK, nranks=p)


# ---- 1. how the pad is resolved -----------------------------------------------------------------------------------------------------
def test_pad_resolution(gpu_pkg, monkeypatch):
    n = 1000   # n16 = 1008

    def lda(pad):
        with gpu_pkg.CGSolver(lda_pad=pad) as s:
            s.generate_lap2d_matrix(n)
            return s.matrix_format(0)[2] / (8.0 * n)

    assert n16(n) == 1008
    assert [lda(pad) for pad in (0, 1, 2, 6, -1)] == [1008, 1010, 1010, 1014, 1024]
    monkeypatch.setenv("CGX_LDA_PAD", "0")
    assert lda(-1) == 1008
    assert lda(2) == 1010          # a configuration value >= 0 wins over the environment variable
    monkeypatch.setenv("CGX_LDA_PAD", "6")
    assert lda(-1) == 1014 and lda(0) == 1008 and lda(16) == 1024
    with gpu_pkg.CGSolver(lda_pad=0) as s:   # n % 16 == 0: the pitch is n itself
        s.generate_lap2d_matrix(1024)
        assert s.matrix_format(0)[2] == 8.0 * 1024 * 1024


# ---- 2. the general K1 alone ------------------------------------------------------------------------------------------------------------
GEMV_SIZES = [16, 1023, 1024, 2033, 2048, 4096, 5200]
GEMV_VARIANTS = tp.VARIANTS + [10825]
_GEMV = {}


def _gemv_problem(n):
    """(A, p, A p in longdouble, |A| |p|), made once per n."""
    if n not in _GEMV:
        rng = np.random.default_rng(20261019 + n)
        A = rng.standard_normal((n, n))
        p = rng.standard_normal(n)
        y_ref = A.astype(LD) @ p.astype(LD)
        for a in (A, p, y_ref):
            a.setflags(write=False)
        _GEMV[n] = (A, p, y_ref, np.abs(A) @ np.abs(p))
    return _GEMV[n]


def _probe(pkg, n, pad, **kw):
    A, p, _, _ = _gemv_problem(n)
    with pkg.CGSolver(lda_pad=pad, **kw) as s:
        s.set_matrix_dense(A)
        assert_pitch(s, n, pad, kw.get("nranks", 1))
        return s.probe_gemv(p)


@pytest.mark.parametrize("variant", GEMV_VARIANTS)
@pytest.mark.parametrize("n", GEMV_SIZES)
def test_gemv_dense_random_without_pad_columns(gpu_pkg, n, variant):
    """probe_gemv on dense random A at pad 0 and 2: test_gemv_dense_random's bounds against the longdouble product, and the bits
    of the default pitch."""
    _, p, y_ref, scale = _gemv_problem(n)
    pap_ref = float(np.sum(p.astype(LD) * y_ref))
    y16, pap16 = _probe(gpu_pkg, n, DEFAULT, gemv_variant=variant)
    for pad in (0, 2):
        y, pap = _probe(gpu_pkg, n, pad, gemv_variant=variant)
        err = np.abs(y.astype(LD) - y_ref)
        bound = 4e-16 * np.sqrt(n) * scale + 1e-300
        print("n=%d variant=%d pad=%d: worst |y - y_ref| / bound %.3f, |pAp - ref| / bound %.3f" % (
            n, variant, pad, float(np.max(err / bound)), abs(pap - pap_ref) / (1e-13 * float(np.sum(np.abs(p * y_ref))))))
        assert np.all(err <= bound), (pad, int(np.argmax(err / bound)))
        assert abs(pap - pap_ref) <= 1e-13 * float(np.sum(np.abs(p * y_ref))), (pad, pap, pap_ref)
        assert np.array_equal(y, y16) and pap == pap16, (pad, int(np.count_nonzero(y != y16)), pap, pap16)


@pytest.mark.parametrize("n,p", [(1024, 3), (2048, 8), (4096, 2)])
def test_gemv_row_blocks_loopback_without_pad_columns(gpu_pkg, n, p):
    _, v, y_ref, _ = _gemv_problem(n)
    yo = y_ref.astype(np.float64)
    y, pap = _probe(gpu_pkg, n, 0, **_shards(gpu_pkg, p))
    assert np.max(np.abs(y - yo)) <= 1e-13 * np.max(np.abs(yo))
    assert abs(pap - float(np.sum(v.astype(LD) * y_ref))) <= 1e-12 * np.sum(np.abs(v * yo))
    y16, pap16 = _probe(gpu_pkg, n, DEFAULT, **_shards(gpu_pkg, p))
    assert np.array_equal(y, y16) and pap == pap16


# ---- 3. the fused forms and K3 through solves on the per-launch path ------------------------------------------------------------------------
ITERS = 12


def _lap2d_solve(pkg, n, pad, p=1, variant=-1):
    mode = None if p == 1 else pkg.COMM_LOOPBACK
    with tp.make(pkg, n, mode, p, variant, ITERS, tol=0.0, lda_pad=pad) as s:
        assert_pitch(s, n, pad, p)
        x = np.zeros(n)
        return x, s.solve(x)


def _check_against_oracle(x, r, xo, ro):
    assert r["iterations"] == ro["iterations"] == ITERS, (r, ro)
    assert np.linalg.norm(x - xo) <= 1e-12 * np.linalg.norm(xo), np.linalg.norm(x - xo) / np.linalg.norm(xo)


@pytest.mark.parametrize("n,p,variant", [(1024, 1, -1), (1023, 1, -1), (1024, 3, -1), (2048, 1, 10442), (2048, 1, 10822), (2048, 1, 20421)])
def test_lap2d_solve_without_pad_columns(gpu_pkg, oracle, n, p, variant):
    x, r = _lap2d_solve(gpu_pkg, n, 0, p, variant)
    _check_against_oracle(x, r, *oracle.solve_lap2d(n, ITERS, 0.0, p))
    same_solve((x, r), _lap2d_solve(gpu_pkg, n, DEFAULT, p, variant), (n, p, variant))


def _hash_solve(pkg, n, pad, p, b, x0):
    with mr._hash_solver(pkg, n, lda_pad=pad, **_shards(pkg, p)) as s:
        assert_pitch(s, n, pad, p)
        s.set_source_term(b)
        s.set_max_iter(ITERS)
        s.tolerance(0.0)
        x = x0.copy()
        return x, s.solve(x)


@pytest.mark.parametrize("n,p", [(1040, 1), (1024, 3)])
def test_dense_hash_solve_with_initial_guess_without_pad_columns(gpu_pkg, oracle, n, p):
    """The SPD hash matrix (every element of A counts) and a nonzero initial guess: the plain K1 of the set-up, the fused K1, K3."""
    A = oracle.hash_rows(n, 0, n, mr.SEED, True, mr._diag(n))
    b = np.cos(np.arange(n, dtype=np.float64))
    x0 = np.sin(np.arange(n) * 0.01)
    x, r = _hash_solve(gpu_pkg, n, 0, p, b, x0)
    _check_against_oracle(x, r, *oracle.solve(A, b, x0, ITERS, 0.0, p))
    same_solve((x, r), _hash_solve(gpu_pkg, n, DEFAULT, p, b, x0), (n, p))


@pytest.mark.parametrize("n", [256, 4096, 100000])
def test_vector_ops_without_pad_elements(gpu_pkg, oracle, n):
    """cgx_probe_vector_ops lays its vectors out at roundup(n, 16) whatever the context's pad: for these n, r's first partial
    sits directly behind element n - 1.  The context's own pitch is asserted on a 16-row problem."""
    assert n % 16 == 0
    out = []
    for pad in (0, DEFAULT):
        with gpu_pkg.CGSolver(lda_pad=pad) as s:
            s.generate_lap2d_matrix(16)
            assert_pitch(s, 16, pad)
            out.append(tp.vector_ops_case(s, oracle, n))
    assert all(np.array_equal(a, b) for a, b in zip(out[0][:3], out[1][:3])) and out[0][3] == out[1][3]


# ---- 4. preconditioners -----------------------------------------------------------------------------------------------------------------------
N_PC = 1024


def _pitch_check(n, pad, p):
    return lambda c: assert_pitch(c, n, pad, p)


@pytest.mark.parametrize("p", [1, 3])
def test_jacobi_dense_scaled_diagonal_without_pad_columns(gpu_pkg, oracle, p):
    """S L S with a diagonal that differs in every row (tests/test_gpu_jacobi_scaled.py): s * x_jacobi equals x_plain bit for
    bit and rel_residual is the host's, at pad 0; x and the reported numbers are those of the default pitch."""
    n, iters = N_PC, 40
    L, s, bt = oracle.generate_lap2d(n), js._scale(n, 31 * n + p), oracle.init_source_term(n)
    kw = dict(gemv_variant=-1, **_shards(gpu_pkg, p))
    xt, xj, rj = js._dense_pair(gpu_pkg, L, s, bt, iters, _pitch_check(n, 0, p), ("pad 0", p), lda_pad=0, **kw)
    xt16, xj16, rj16 = js._dense_pair(gpu_pkg, L, s, bt, iters, _pitch_check(n, DEFAULT, p), ("default", p), **kw)
    assert np.array_equal(xt, xt16)
    same_solve((xj, rj), (xj16, rj16), p)


@pytest.mark.parametrize("p", [1, 3])
def test_jacobi_csr_scaled_diagonal_without_pad_elements(gpu_pkg, oracle, p):
    n, iters = N_PC, 40
    assert_pitch_on_dense_twin(gpu_pkg, n, 0, p)
    indptr, indices, data = tc.lap2d_csr(n)
    rows = js._csr_rows(indptr)
    s = js._scale(n, 7 * n + p)
    bt = oracle.init_source_term(n)
    scaled = s[rows] * data * s[indices]
    xt, _ = js._csr_run(gpu_pkg, p, 0, (indptr, indices, data), bt, iters, False, lda_pad=0)
    xj, rj = js._csr_run(gpu_pkg, p, 0, (indptr, indices, scaled), s * bt, iters, True, lda_pad=0)
    js._assert_same_bits(s, xj, xt, ("csr pad 0", p))
    ax, aax = js._csr_products(rows, indices, scaled, xj, n)
    js._check_rel_residual(rj, ax, aax, s * bt, 5, ("csr pad 0", p))
    same_solve((xj, rj), js._csr_run(gpu_pkg, p, 0, (indptr, indices, scaled), s * bt, iters, True), p)


def _block_jacobi(pkg, name, block, pad):
    A, b = bj._matrix(name)
    with bj._solver(pkg, "dense", 1, -1, lda_pad=pad) as c:
        bj._load(c, "dense", A)
        assert_pitch(c, len(b), pad)
        c.set_preconditioner("jacobi", block=block)
        x, res = bj._solve(c, b, ITERS)
        return c._probe_precond_blocks(), x, res


@pytest.mark.parametrize("block", [2, 16, 256])
@pytest.mark.parametrize("name", ["lap2d1024", "lap2d1000"])   # lda == n: W's columns touch; lda = 1008: the last block is cut at n
def test_block_jacobi_without_pad_columns(gpu_pkg, name, block):
    A, _ = bj._matrix(name)
    W, x, res = _block_jacobi(gpu_pkg, name, block, 0)
    bj._check_inverse(W, A, block, (name, "pad 0"))
    want = bj._reference(name, block, ITERS, 0.0, (ITERS,))["xs"][ITERS]
    err = float(np.linalg.norm(x - want) / np.linalg.norm(want))
    print("block Jacobi %s block %d pad 0: |x - x_ref| / |x_ref| = %.3e" % (name, block, err))
    assert res["iterations"] == ITERS and err <= bj.REL_BOUND, (res, err)
    W16, x16, res16 = _block_jacobi(gpu_pkg, name, block, DEFAULT)
    assert np.array_equal(W, W16)
    same_solve((x, res), (x16, res16), (name, block))


@pytest.mark.parametrize("n,rank", [(1024, 64), (1024, 256), (1008, 100), (1101, 64)])
def test_pivoted_cholesky_factor_and_apply_without_pad_columns(gpu_pkg, n, rank):
    f = pv._device_factor(gpu_pkg, n, rank, check=_pitch_check(n, 0, 1), lda_pad=0)
    pv._check_factor(f, n, rank)
    pv._check_apply(f, n, rank)
    f16 = pv._device_factor(gpu_pkg, n, rank, check=_pitch_check(n, DEFAULT, 1))
    assert np.array_equal(f["piv"], f16["piv"]) and np.array_equal(f["L"], f16["L"])
    assert f["delta"] == f16["delta"] and f["fixed"] == f16["fixed"]
    for name in f["z"]:
        assert np.all(np.isfinite(f["z"][name])) and np.array_equal(f["z"][name], f16["z"][name]), name


def test_pivoted_cholesky_solve_without_pad_columns(gpu_pkg):
    n, rank = 1024, 64
    out = []
    for pad in (0, DEFAULT):
        with pv._solver(gpu_pkg, n, lda_pad=pad) as s:
            assert_pitch(s, n, pad)
            s.set_preconditioner("pivchol", rank=rank)
            x = np.zeros(n)
            res = s.solve(x)
            _, L, delta = s._probe_precond_lowrank()
        out.append((x, res, L, delta))
    x, res, L, delta = out[0]
    pv._check_solve(x, res, n, L, delta)
    same_solve((x, res), out[1][:2])
    assert np.array_equal(L, out[1][2]) and delta == out[1][3]


# ---- 5. several right-hand sides and shifts -------------------------------------------------------------------------------------------------------
WIDTHS = (1, 2, 4, 5, 8, 11, 16)


@pytest.mark.parametrize("n", [256, 257, 512])
def test_probe_gemv_multi_without_pad_elements(gpu_pkg, oracle, n):
    """test_probe_hash_every_row's check at pad 0: the columns of the block touch, width 4 exactly and widths 8 and 16 partly filled."""
    rng = np.random.default_rng(n)
    blocks = [rng.standard_normal((k, n)) for k in WIDTHS]
    out = {}
    for pad in (0, DEFAULT):
        with mr._hash_solver(gpu_pkg, n, symmetric=False, lda_pad=pad) as s:
            assert_pitch(s, n, pad)
            out[pad] = [s.probe_gemv_multi(P) for P in blocks]
    for P, (Y, pap), (Y16, pap16) in zip(blocks, out[0], out[DEFAULT]):
        k = P.shape[0]
        for j in range(k):
            rows, y_ref, abs_ap = oracle.hash_gemv_longdouble(n, mr.SEED, P[j])
            assert oracle.gemv_rows_outside(Y[j][rows], y_ref, abs_ap, n).size == 0, (k, j)
            ref = float(np.sum(P[j].astype(LD) * y_ref))
            bound = 4e-16 * np.sqrt(n) * float(np.abs(P[j]) @ abs_ap) * 4
            assert abs(pap[j] - ref) <= bound, (k, j, pap[j], ref)
        assert np.array_equal(Y, Y16) and np.array_equal(pap, pap16), k


def _solve_multi(pkg, n, pad, B, X0):
    with mr._hash_solver(pkg, n, lda_pad=pad) as s:
        assert_pitch(s, n, pad)
        s.set_max_iter(ITERS)
        s.tolerance(0.0)
        return s.solve_multi(B, X0)


@pytest.mark.parametrize("n,k", [(1024, 16), (1023, 3)])
def test_solve_multi_without_pad_elements(gpu_pkg, oracle, n, k):
    A = oracle.hash_rows(n, 0, n, mr.SEED, True, mr._diag(n))
    B = mr._rhs_block(oracle, A, n, k)
    X0 = mr._x0_block(n, k)   # column 1 starts from a nonzero guess
    assert np.any(X0[1] != 0.0)
    X, res = _solve_multi(gpu_pkg, n, 0, B, X0)
    mr._check_columns(oracle, A, B, X0, X, res, ITERS, 0.0)
    # a column does not see its neighbours: other right-hand sides and guesses beside it leave its result as it is
    j = 1
    B2 = np.array(B[::-1]) * 3.0 + 1.0
    X2 = np.array(X0[::-1]) + 0.25
    B2[j], X2[j] = B[j], X0[j]
    Xn, resn = _solve_multi(gpu_pkg, n, 0, B2, X2)
    same_solve((X[j], res[j]), (Xn[j], resn[j]), ("neighbours", j))
    assert not np.array_equal(X[j - 1], Xn[j - 1])
    X16, res16 = _solve_multi(gpu_pkg, n, DEFAULT, B, X0)
    for c in range(k):
        same_solve((X[c], res[c]), (X16[c], res16[c]), c)


def _solve_shifted(pkg, n, storage, pad, shifts):
    with sh._solver(pkg, "lap2d", n, storage, lda_pad=pad) as s:
        if storage == "dense":
            assert_pitch(s, n, pad)
        s.set_max_iter(ITERS)
        s.tolerance(0.0)
        x = np.zeros(n)
        r = s.solve(x)
        X, res = s.solve_shifted(shifts)
    return x, r, X, res


@pytest.mark.parametrize("storage", ["dense", "csr"])
def test_solve_shifted_without_pad_elements(gpu_pkg, oracle, storage):
    n = 1024
    shifts = [float(v) for v in np.linspace(0.0, 100.0, 16)]
    if storage == "csr":
        assert_pitch_on_dense_twin(gpu_pkg, n, 0)
    x, r, X, res = _solve_shifted(gpu_pkg, n, storage, 0, shifts)
    assert X.shape == (16, n)
    for j, sigma in enumerate(shifts):
        xo, ro = sh._reference(oracle, "lap2d", n, sigma, ITERS, 0.0)
        err = np.linalg.norm(X[j] - xo) / np.linalg.norm(xo)
        assert res[j]["iterations"] == ro["iterations"] == ITERS, (sigma, res[j], ro)
        assert err <= 1e-12, (sigma, err)
    # sigma = 0 is cgx_solve at the same pitch, bit for bit
    assert shifts[0] == 0.0 and np.array_equal(X[0], x)
    assert res[0]["iterations"] == r["iterations"] and res[0]["residual_prev"] == r["residual_prev"], (res[0], r)
    x16, r16, X16, res16 = _solve_shifted(gpu_pkg, n, storage, DEFAULT, shifts)
    same_solve((x, r), (x16, r16), storage)
    for j in range(16):
        same_solve((X[j], res[j]), (X16[j], res16[j]), (storage, j))


def _solve_minres(pkg, oracle, kind, n, storage, pad):
    _, _, S = mn._problem(oracle, kind, n)
    with mn._solver(pkg, oracle, kind, n, storage, lda_pad=pad) as s:
        if storage == "dense":
            assert_pitch(s, n, pad)
        s.set_max_iter(ITERS)
        s.tolerance(0.0)
        return s.solve_minres(S)


# lda == n and 256 K1 partials (the first load slot of fold_pap exactly full) | one pad element | lda == n on CSR
@pytest.mark.parametrize("kind,n,storage", [("hash0", 1024, "dense"), ("hash0", 1023, "dense"), ("lap2d", 1008, "csr")])
def test_solve_minres_without_pad_elements(gpu_pkg, oracle, kind, n, storage):
    """cgx_solve_minres with 8 shifts of both signs: the sixteen lda-long columns of X, D[0], D[1] and Y and the two recurrence
    vectors of its side block lie end to end, and k_minres_init writes rows n .. lda - 1 of each.  tests/test_gpu_minres.py's bars
    against tests/minres_reference.py, and the default pitch's bits: the rows behind n hold exact zeros at every pitch."""
    assert pitch(n, 0) == n16(n) and (n % 16 == 0 or pitch(n, 0) == n + 1)
    if storage == "csr":
        assert_pitch_on_dense_twin(gpu_pkg, n, 0)
    A, b, S = mn._problem(oracle, kind, n)
    assert len(S) == 8
    X, res = _solve_minres(gpu_pkg, oracle, kind, n, storage, 0)
    absA = np.abs(A)
    mn._check_against_reference(X, res, mn._reference(oracle, kind, n, S, ITERS, 0.0), lambda x: A @ x, lambda x: absA @ x, b, S, ITERS,
                                6 if kind == "lap2d" else n, "minres pad 0 %s n=%d %s" % (kind, n, storage))
    X16, res16 = _solve_minres(gpu_pkg, oracle, kind, n, storage, DEFAULT)
    for j in range(len(S)):
        same_solve((X[j], res[j]), (X16[j], res16[j]), (kind, n, storage, S[j]))


# ---- 6. the symmetric K1 (variant 6), the sparse K1s ----------------------------------------------------------------------------------------------------
GRID_WALK = 60000
_SYM = {}


def _symv_probe(pkg, n, pad, variant, seed, pvec):
    with pkg.CGSolver(lda_pad=pad, gemv_variant=variant) as s:
        s.generate_lap2d_matrix(n)
        assert_pitch(s, n, pad)
        s.probe_fill_matrix_hash(seed, symmetric=True)
        plan = s.gemv_plan()
        assert plan["variant"] == 6, plan
        y, pap = s.probe_gemv(pvec)
    assert np.all(np.isfinite(y))
    return plan, y, pap


def _symv_reference(pkg, oracle, n, seed, pvec):
    """Per n, once: the longdouble product and the default pitch's result."""
    if n not in _SYM:
        oracle.set_threads(16)
        try:
            ref = oracle.hash_gemv_longdouble(n, seed, pvec, symmetric=True)
        finally:
            oracle.set_threads(1)
        _SYM[n] = (ref, _symv_probe(pkg, n, DEFAULT, 0, seed, pvec))
    return _SYM[n]


# lda == n and a ragged last tile | odd n, lda = 16400 | odd n, two pad columns more
@pytest.mark.parametrize("n,pad", [(16400, 0), (16385, 0), (16385, 2)])
def test_symmetric_k1_without_pad_columns(gpu_pkg, oracle, n, pad):
    seed = sp.SEED + n
    pvec = np.random.default_rng(n).standard_normal(n)
    plan, y, pap = _symv_probe(gpu_pkg, n, pad, 0, seed, pvec)
    (rows, yr, abs_ap), (_, y16, pap16) = _symv_reference(gpu_pkg, oracle, n, seed, pvec)
    sp._assert_rows(oracle, n, plan, y, rows, yr, abs_ap)
    pap_ref = np.sum(pvec.astype(LD) * yr)
    tol = np.sum(np.abs(pvec) * 4e-16 * np.sqrt(n) * abs_ap) + 4e-16 * np.sqrt(n) * np.sum(np.abs(pvec * y))
    assert abs(pap - pap_ref) <= tol, (plan, float(pap - pap_ref), float(tol))
    plan_w, y_w, pap_w = _symv_probe(gpu_pkg, n, pad, GRID_WALK, seed, pvec)   # the same kernel on the grid of 4 workgroups per CU
    assert plan_w["grid"] < plan["grid"] and plan_w["U"] > plan["U"], (plan, plan_w)
    assert np.array_equal(y, y_w) and pap == pap_w
    assert np.array_equal(y, y16) and pap == pap16


def test_symmetric_k1_fused_solve_without_pad_columns(gpu_pkg, oracle):
    n, iters = 16400, 5
    seed = sp.SEED + 2 * n
    out = []
    for pad in (0, DEFAULT):
        with gpu_pkg.CGSolver(lda_pad=pad) as s:
            s.generate_lap2d_matrix(n)
            assert_pitch(s, n, pad)
            s.probe_fill_matrix_hash(seed, symmetric=True, diag=sp._diag(n))
            assert s.gemv_plan()["variant"] == 6
            s.set_source_term(sp._rhs(n))
            s.set_max_iter(iters)
            s.tolerance(0.0)
            x = np.zeros(n)
            out.append((x, s.solve(x)))
    xo, ro = sp._oracle_solve(oracle, sp._host_spd(oracle, n, seed), sp._rhs(n), iters)
    assert out[0][1]["iterations"] == iters
    sp._close(out[0][0], xo, out[0][1], ro)
    same_solve(out[0], out[1])


_LANES = {}


@pytest.mark.parametrize("p", [1, 3])
@pytest.mark.parametrize("L", [1, 8, 64])
def test_csr_lanes_without_pad_elements(gpu_pkg, L, p):
    n = 3008
    assert n % 16 == 0
    assert_pitch_on_dense_twin(gpu_pkg, n, 0, p)
    if L not in _LANES:
        _LANES[L] = tc.lanes_problem(n, L)
    A, v, yo = _LANES[L]
    out = []
    for pad in (0, DEFAULT):
        with tc.solver(gpu_pkg, p, gemv_variant=70000 + L, lda_pad=pad) as s:
            s.set_matrix_csr(*tc.dense_to_csr(A))
            assert s.gemv_plan()["R"] == L
            out.append(s.probe_gemv(v))
    tc.check_lanes_product(A, v, yo, *out[0])
    assert np.array_equal(out[0][0], out[1][0]) and out[0][1] == out[1][1]


def _banded(pkg, n, pad, p, variant, v):
    """probe_gemv, then a fixed-iteration solve, on banded storage."""
    mode = None if p == 1 else pkg.COMM_LOOPBACK
    with tb.make(pkg, n, mode, p, ITERS, tol=0.0, gemv_variant=variant, lda_pad=pad) as s:
        assert s.gemv_plan()["variant"] == 3 and s.gemv_plan()["light"] == (variant == tb.K1B_WINDOWS), s.gemv_plan()
        y, pap = s.probe_gemv(v)
        x = np.zeros(n)
        return y, pap, x, s.solve(x)


# (4096, 1): column n - 1 of rows n - 2 and n - 66 is the upper half of a pair whose other half would be element n.
# (48, 16): three rows per shard, the last shard's last row is an odd one: its own pair would begin at element n - 1.
@pytest.mark.parametrize("variant", [tb.K1B_DIRECT, tb.K1B_WINDOWS])
@pytest.mark.parametrize("n,p", [(4096, 1), (48, 16)])
def test_banded_k1_without_pad_elements(gpu_pkg, oracle, n, p, variant):
    """Both forms of K1b on lap2d: the product against oracle.gemv with tests/test_gpu_banded.py's bounds, the fused form through a
    solve against the oracle, and the default pitch's bits.  At lda == n both forms used to touch element n of p (module header)."""
    assert n % 16 == 0
    assert_pitch_on_dense_twin(gpu_pkg, n, 0, p)
    v = np.random.default_rng(n + p).standard_normal(n)
    y, pap, x, r = _banded(gpu_pkg, n, 0, p, variant, v)
    yo = oracle.gemv(oracle.generate_lap2d(n), v)
    assert np.max(np.abs(y - yo)) <= 1e-14 * np.max(np.abs(yo))
    assert abs(pap - v @ yo) <= 1e-12 * np.sum(np.abs(v * yo))
    _check_against_oracle(x, r, *oracle.solve_lap2d(n, ITERS, 0.0, p))
    y16, pap16, x16, r16 = _banded(gpu_pkg, n, DEFAULT, p, variant, v)
    assert np.array_equal(y, y16) and pap == pap16
    same_solve((x, r), (x16, r16), (n, p, variant))
