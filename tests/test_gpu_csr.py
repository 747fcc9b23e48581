"""Opt-in CSR storage (cgx_config.matrix_format = CGX_MATRIX_CSR) against the dense and banded paths,
the CPU oracle, the reference's recorded outputs and a numpy longdouble restatement.

1. Storage: the densified CSR rows equal the dense context's bit for bit (generator, .mtx files, caller's dense matrix).
2. Mat-vec: L = 1 equals banded 30001 bit for bit; every L agrees with longdouble A p.
3. Solve parity with the banded tests' tolerances; begin / steps / end equals the one-shot solve.
4. Matrices neither dense nor banded storage can take: a permuted lap2d at n = 2^20, a skewed SPD matrix.
5. cgx_set_matrix_csr validation.  6. Jacobi on CSR.  7. Refusals and plan.  8. CLI, RCCL (fake) transport.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "conjugate-gradient_amd", "cgsolver")
BAD_ARG, UNSUPPORTED = 1, 7
LANES = (1, 2, 4, 8, 16, 32, 64)


def rel(a, b):
    return abs(a - b) / abs(b)


def lap2d_csr(n, perm=None):
    """The generator's matrix (cg.cc:159-188) as CSR in numpy; perm: new index of old row i (A' = P A P^T)."""
    inc = int(np.floor(np.sqrt(n)))
    i = np.arange(n, dtype=np.int64)
    rows, cols, vals = [i], [i], [np.full(n, 4.0)]
    for off, ok in ((-1, i > 0), (1, i < n - 1), (-(inc + 1), i > inc), (inc + 1, i < n - 1 - inc)):
        rows.append(i[ok])
        cols.append(i[ok] + off)
        vals.append(np.full(int(ok.sum()), -1.0))
    r, c, v = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
    if perm is not None:
        r, c = perm[r], perm[c]
    order = np.lexsort((c, r))
    r, c, v = r[order], c[order], v[order]
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.add.at(indptr, r + 1, 1)
    return np.cumsum(indptr), c.astype(np.int32), v


def csr_to_dense(indptr, indices, data, n):
    A = np.zeros((n, n))
    for i in range(n):
        A[i, indices[indptr[i]:indptr[i + 1]]] = data[indptr[i]:indptr[i + 1]]
    return A


def dense_to_csr(A):
    indptr = np.zeros(A.shape[0] + 1, dtype=np.int64)
    nzr, nzc = np.nonzero(A)
    np.add.at(indptr, nzr + 1, 1)
    return np.cumsum(indptr), nzc.astype(np.int32), A[nzr, nzc]


def rows_of(s, p):
    return np.vstack([s.probe_matrix_rows(q)[0] for q in range(p)])


def solver(pkg, p=1, fmt=None, **kw):
    mode = pkg.COMM_SELF if p == 1 else pkg.COMM_LOOPBACK
    return pkg.CGSolver(comm_mode=mode, nranks=p, matrix_format=pkg.MATRIX_CSR if fmt is None else fmt, **kw)


def solve(s, n, max_iter=None, tol=None, b=None, x0=None):
    if max_iter is not None:
        s.set_max_iter(max_iter)
    if tol is not None:
        s.tolerance(tol)
    if b is None:
        s.init_source_term(1.0 / n)
    else:
        s.set_source_term(b)
    x = np.zeros(n) if x0 is None else x0.copy()
    r = s.solve(x)
    return x, r


# ---- 1. storage ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,p", [(1, 1), (3, 1), (17, 1), (4096, 1), (4096, 3), (5, 8)])
def test_generator_storage_equals_dense(gpu_pkg, n, p):
    with solver(gpu_pkg, p, fmt=gpu_pkg.MATRIX_DENSE) as d:
        d.generate_lap2d_matrix(n)
        dense = [d.probe_matrix_rows(q) for q in range(p)]
    with solver(gpu_pkg, p) as s:
        s.generate_lap2d_matrix(n)
        for q in range(p):
            A, row0 = s.probe_matrix_rows(q)
            rows = A.shape[0]
            assert row0 == dense[q][1] and rows == dense[q][0].shape[0]
            assert np.array_equal(A.view(np.uint64), dense[q][0].view(np.uint64)), q
            nnz = int(np.count_nonzero(dense[q][0]))
            assert s.matrix_nnz(q) == nnz
            assert s.matrix_format(q) == (2, [], 12.0 * nnz + 8.0 * (rows + 1))


def _mtx(tmp_path, name, n, entries, sym):
    f = tmp_path / name
    kind = "symmetric" if sym else "general"
    f.write_text("%%%%MatrixMarket matrix coordinate real %s\n%d %d %d\n" % (kind, n, n, len(entries)) +
                 "".join("%d %d %r\n" % (i + 1, j + 1, v) for i, j, v in entries))
    return str(f)


def _mtx_cases(tmp_path):
    rng = np.random.default_rng(5)
    n = 40
    ent = [(int(i), int(j), float(v)) for i, j, v in zip(rng.integers(0, n, 300), rng.integers(0, n, 300), rng.standard_normal(300))]
    ent += [(3, 7, 1.5), (3, 7, -2.25), (3, 7, 0.0), (9, 9, 0.0), (11, 2, 5.0), (11, 2, 6.0)]   # duplicates, explicit zeros
    ent = [e for e in ent if e[0] not in (20, 21, 33)]                                             # empty rows
    low = [(max(i, j), min(i, j), v) for i, j, v in ent]
    return [_mtx(tmp_path, "gen.mtx", n, ent, False), _mtx(tmp_path, "sym.mtx", n, low, True)]


@pytest.mark.parametrize("p", [1, 3])
def test_mtx_storage_equals_dense_reader(gpu_pkg, mtx_path, tmp_path, p):
    for path in _mtx_cases(tmp_path) + [mtx_path]:
        with solver(gpu_pkg, p, fmt=gpu_pkg.MATRIX_DENSE) as d:
            d.read_matrix(path)
            want = rows_of(d, p)
        with solver(gpu_pkg, p) as s:
            s.read_matrix(path)
            got = rows_of(s, p)
            nnz = sum(s.matrix_nnz(q) for q in range(p))
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), path
        # every assigned position is stored (an exact 0 included): at least the dense non-zeros, at most the file's entries x 2
        assert np.count_nonzero(want) <= nnz
        if path == mtx_path:
            assert nnz == np.count_nonzero(want)


def test_caller_dense_matrix_is_packed(gpu_pkg, oracle):
    n = 600
    rng = np.random.default_rng(11)
    A = oracle.generate_lap2d(n) + np.diag(rng.uniform(0.0, 1.0, n))
    A[5, 300] = A[300, 5] = 0.25
    with solver(gpu_pkg, 3) as s:
        s.set_matrix_dense(A)
        assert np.array_equal(rows_of(s, 3), A)
        assert sum(s.matrix_nnz(q) for q in range(3)) == np.count_nonzero(A)


# ---- 2. mat-vec ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,p", [(4096, 1), (4096, 3), (65536, 1), (1000, 7)])
def test_lane1_equals_banded_direct_form(gpu_pkg, n, p):
    v = np.random.default_rng(n).standard_normal(n)
    out = []
    for fmt, variant in ((gpu_pkg.MATRIX_CSR, 70001), (gpu_pkg.MATRIX_BANDED, 30001)):
        with solver(gpu_pkg, p, fmt=fmt, gemv_variant=variant) as s:
            s.generate_lap2d_matrix(n)
            out.append(s.probe_gemv(v))
    assert np.array_equal(out[0][0], out[1][0])


def lanes_problem(n, L):
    """(A, v, A v in longdouble): 2 % filled rows, every 97th row 60 % filled, one empty row, a dominant diagonal."""
    rng = np.random.default_rng(L)
    A = np.where(rng.random((n, n)) < 0.02, rng.standard_normal((n, n)), 0.0)
    A[::97, :] = np.where(rng.random((len(A[::97]), n)) < 0.6, rng.standard_normal((len(A[::97]), n)), 0.0)   # long rows
    A[50, :] = 0.0                                                                                              # an empty row
    A += np.diag(np.where(np.arange(n) == 50, 0.0, 100.0))   # p.Ap dominated by positive terms: a relative bound is meaningful
    v = rng.standard_normal(n)
    return A, v, A.astype(np.longdouble) @ v.astype(np.longdouble)


def check_lanes_product(A, v, yo, y, pap):
    bound = 2e-14 * (np.abs(A) @ np.abs(v))
    assert np.all(np.abs(y - yo.astype(np.float64)) <= bound + 1e-300)
    assert rel(pap, float(v.astype(np.longdouble) @ yo)) < 1e-13


@pytest.mark.parametrize("L", LANES)
@pytest.mark.parametrize("p", [1, 3])
def test_every_lane_count_against_longdouble(gpu_pkg, L, p):
    A, v, yo = lanes_problem(3000, L)
    with solver(gpu_pkg, p, gemv_variant=70000 + L) as s:
        s.set_matrix_csr(*dense_to_csr(A))
        assert s.gemv_plan()["R"] == L
        y, pap = s.probe_gemv(v)
    check_lanes_product(A, v, yo, y, pap)


def test_row_result_depends_on_lanes_only(gpu_pkg):
    """A row's sum is a function of (row, L): the same on 1, 2 and 5 shards."""
    n = 5000
    v = np.random.default_rng(3).standard_normal(n)
    for L in (1, 8, 64):
        ys = []
        for p in (1, 2, 5):
            with solver(gpu_pkg, p, gemv_variant=70000 + L) as s:
                s.generate_lap2d_matrix(n)
                ys.append(s.probe_gemv(v)[0])
        assert all(np.array_equal(ys[0], y) for y in ys[1:]), L


# ---- 3. solve parity ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,p", [(1024, 1), (4096, 1), (65536, 1), (1024, 2), (4096, 3), (65536, 5)])
def test_solve_matches_banded_oracle(gpu_pkg, oracle, n, p):
    max_iter = 150   # below n = 1024's convergence (176 iterations at tol 1e-10)
    with solver(gpu_pkg, p) as s:
        s.generate_lap2d_matrix(n)
        x, r = solve(s, n, max_iter)
    xo, ro = oracle.solve_lap2d_banded(n, max_iter, 1e-10, p)
    assert r["iterations"] == ro["iterations"] == max_iter
    assert rel(r["residual_prev"], ro["residual_prev"]) < 1e-6
    assert np.linalg.norm(x - xo) / np.linalg.norm(xo) < 1e-12
    assert rel(r["x_norm"], ro["x_norm"]) < 1e-12


@pytest.mark.parametrize("n,p", [(1024, 1), (1000, 3)])
def test_converged_solve(gpu_pkg, oracle, n, p):
    with solver(gpu_pkg, p) as s:
        s.generate_lap2d_matrix(n)
        x, r = solve(s, n)
    xo, ro = oracle.solve_lap2d(n, None, 1e-10, p)
    assert r["converged"] and r["residual_last"] < 1e-10 <= r["residual_prev"]
    assert np.linalg.norm(x - xo) / np.linalg.norm(xo) < 1e-12
    assert abs(r["iterations"] - ro["iterations"]) <= 0.15 * ro["iterations"]


@pytest.mark.parametrize("p", [1, 8])
def test_config3_n32768_500_iterations_matches_reference(gpu_pkg, reference_probe, p):
    row = [q for q in reference_probe["generated_large"] if q["n"] == 32768][0]
    with solver(gpu_pkg, p) as s:
        s.generate_lap2d_matrix(32768)
        x, r = solve(s, 32768, 500)
        fmt, offs, nbytes = s.matrix_format(0)
    assert fmt == 2 and offs == [] and nbytes < 2.5e6          # 8 GiB as a dense block
    assert r["iterations"] == row["k"]
    assert rel(r["residual_prev"], row["residual"]) < 1e-6
    assert rel(r["x_norm"], row["x_norm"]) < 1e-12
    assert rel(r["rel_residual"], row["rel_residual"]) < 1e-5
    for i, v in row["x_samples"].items():
        assert rel(x[int(i)], v) < 1e-12, i


@pytest.mark.parametrize("p", [1, 3])
def test_cut_solve_equals_one_shot(gpu_pkg, p):
    n = 4096
    with solver(gpu_pkg, p) as s:
        s.generate_lap2d_matrix(n)
        x1, r1 = solve(s, n, 150, 0.0)
        s.init_source_term(1.0 / n)
        s.solve_begin(np.zeros(n))
        done = 0
        while done < 150:
            s.solve_steps(min(7, 150 - done))
            done += min(7, 150 - done)
        x2 = np.zeros(n)
        r2 = s.solve_end(x2)
    assert np.array_equal(x1.view(np.uint64), x2.view(np.uint64))
    assert r1["iterations"] == r2["iterations"] and r1["residual_prev"] == r2["residual_prev"]


# ---- 4. beyond dense and banded storage ---------------------------------------------------------------------------------
def test_permuted_lap2d_at_2_pow_20(gpu_pkg, oracle, tmp_path):
    n = 1 << 20
    perm = np.random.default_rng(20261016).permutation(n)
    indptr, indices, data = lap2d_csr(n, perm)
    # banded storage refuses the permuted matrix (existing behaviour): far more than 64 diagonals
    head = indptr[4096]
    f = tmp_path / "perm.mtx"
    r_ = np.repeat(np.arange(4096), np.diff(indptr[:4097]))
    with open(f, "w") as fh:
        fh.write("%%%%MatrixMarket matrix coordinate real general\n%d %d %d\n" % (n, n, head))
        np.savetxt(fh, np.column_stack([r_ + 1, indices[:head] + 1, data[:head].astype(np.int64)]), fmt="%d")
    with gpu_pkg.CGSolver(matrix_format=gpu_pkg.MATRIX_BANDED) as s:
        with pytest.raises(gpu_pkg.CgxError) as e:
            s.read_matrix(str(f))
        assert e.value.status == UNSUPPORTED and "diagonals" in str(e.value)
    b = oracle.init_source_term(n)
    bp = np.empty(n)
    bp[perm] = b
    with solver(gpu_pkg) as s:
        s.set_matrix_csr(indptr, indices, data)
        assert s.matrix_nnz() == len(data)
        x, r = solve(s, n, 200, 0.0, b=bp)
    xo, ro = oracle.solve_lap2d_banded(n, 200, 0.0, 1)
    assert r["iterations"] == 200
    assert np.linalg.norm(x[perm] - xo) / np.linalg.norm(xo) < 1e-9


def _skewed_spd(n, seed=7):
    rng = np.random.default_rng(seed)
    cnt = rng.integers(3, 10, n)
    heavy = rng.choice(n, n // 100, replace=False)
    cnt[heavy] = rng.integers(500, 2001, len(heavy))
    r = np.repeat(np.arange(n), cnt)
    c = rng.integers(0, n, len(r))
    v = -rng.uniform(0.1, 1.0, len(r))
    keep = r != c
    lo, hi = np.minimum(r, c)[keep], np.maximum(r, c)[keep]   # summed once per unordered pair, then mirrored: exactly symmetric
    uk, inv = np.unique(lo * n + hi, return_inverse=True)
    half = np.zeros(len(uk))
    np.add.at(half, inv, v[keep])
    r, c, vals = np.concatenate([uk // n, uk % n]), np.concatenate([uk % n, uk // n]), np.concatenate([half, half])
    diag = np.zeros(n)
    np.add.at(diag, r, -vals)
    r = np.concatenate([r, np.arange(n)])
    c = np.concatenate([c, np.arange(n)])
    vals = np.concatenate([vals, diag + 1.0])
    order = np.lexsort((c, r))
    r, c, vals = r[order], c[order], vals[order]
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.add.at(indptr, r + 1, 1)
    return np.cumsum(indptr), c.astype(np.int32), vals


class _CsrLike:
    """What scipy.sparse.csr_matrix offers, without importing scipy."""

    def __init__(self, indptr, indices, data, n):
        self.indptr, self.indices, self.data, self.shape = indptr, indices, data, (n, n)


def test_skewed_spd_matches_dense(gpu_pkg):
    n = 16000
    indptr, indices, data = _skewed_spd(n)
    try:
        import scipy.sparse as sp
        mat = sp.csr_matrix((data, indices, indptr), shape=(n, n))
    except ImportError:
        mat = _CsrLike(indptr, indices, data, n)
    out = []
    with solver(gpu_pkg) as s:
        s.set_matrix_csr(mat)
        out.append(solve(s, n, n, 1e-8))
    with solver(gpu_pkg, fmt=gpu_pkg.MATRIX_DENSE) as d:
        d.set_matrix_dense(csr_to_dense(indptr, indices, data, n))
        out.append(solve(d, n, n, 1e-8))
    (xc, rc), (xd, rd) = out
    assert rc["converged"] and rd["converged"]
    assert abs(rc["iterations"] - rd["iterations"]) <= 1
    assert rc["rel_residual"] < 1e-9
    assert np.linalg.norm(xc - xd) / np.linalg.norm(xd) < 1e-8


# ---- 5. cgx_set_matrix_csr validation -----------------------------------------------------------------------------------
def test_set_matrix_csr_validation(gpu_pkg):
    ip, ix, dv = lap2d_csr(100)
    bad = []
    c = ix.copy(); c[ip[10]], c[ip[10] + 1] = c[ip[10] + 1], c[ip[10]]; bad.append((ip, c, dv, 100, "row 10"))   # unsorted
    c = ix.copy(); c[ip[12] + 1] = c[ip[12]]; bad.append((ip, c, dv, 100, "row 12"))                            # duplicate
    c = ix.copy(); c[ip[99 + 1] - 1] = 100; bad.append((ip, c, dv, 100, "row 99"))                              # out of range
    c = ix.copy(); c[ip[3]] = -1; bad.append((ip, c, dv, 100, "row 3"))
    q = ip.copy(); q[40] = q[41] + 1; bad.append((q, ix, dv, 100, "row 40"))                                   # not monotone
    q = ip.copy(); q[0] = 1; bad.append((q, ix, dv, 100, "row 0"))                                             # not from 0
    with solver(gpu_pkg) as s:
        for indptr, col, val, n, what in bad:
            with pytest.raises(gpu_pkg.CgxError) as e:
                s.set_matrix_csr(indptr, col, val, n=n)
            assert e.value.status == BAD_ARG and what in str(e.value), (what, str(e.value))
        for n in (0, -5):
            with pytest.raises(gpu_pkg.CgxError) as e:
                s.set_matrix_csr(ip, ix, dv, n=n)
            assert e.value.status == BAD_ARG
        assert gpu_pkg.cgx.lib().cgx_set_matrix_csr(s._h, 100, None, None, None) == BAD_ARG
        s.set_matrix_csr(ip, ix, dv)                     # still usable: a valid matrix solves
        x, r = solve(s, 100, 50, 0.0)
        assert r["iterations"] == 50 and np.all(np.isfinite(x))
    with solver(gpu_pkg, fmt=gpu_pkg.MATRIX_DENSE) as d:
        with pytest.raises(gpu_pkg.CgxError) as e:
            d.set_matrix_csr(ip, ix, dv)
        assert e.value.status == UNSUPPORTED


def test_explicit_zeros_are_stored(gpu_pkg):
    ip, ix, dv = lap2d_csr(64)
    dv = dv.copy()
    dv[ip[5] + 1] = 0.0
    with solver(gpu_pkg) as s:
        s.set_matrix_csr(ip, ix, dv)
        assert s.matrix_nnz() == len(dv)


# ---- 6. Jacobi on CSR ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p,L", [(1, 0), (3, 0), (1, 70016), (3, 70002)])
def test_jacobi_power_of_two_diagonal_gives_the_plain_bits(gpu_pkg, p, L):
    n = 4096
    out = []
    for jac in (None, "jacobi"):
        with solver(gpu_pkg, p, gemv_variant=L) as s:
            s.generate_lap2d_matrix(n)
            s.set_preconditioner(jac)
            out.append(solve(s, n, 120, 0.0))
    (x0, r0), (x1, r1) = out
    assert np.array_equal(x0.view(np.uint64), x1.view(np.uint64))
    for k in ("iterations", "residual_prev", "residual_last", "x_norm"):
        assert r0[k] == r1[k], k


@pytest.mark.parametrize("tagged,port", [(0, 29791), (1, 29792)])
def test_jacobi_p2p_processes_give_the_plain_bits(tmp_path, tagged, port):
    out = tmp_path / "p2p_csr.txt"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "3", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "p2p_csr_worker.py"), "3000", "80", str(out), str(tagged)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=420, env=dict(os.environ, OMP_NUM_THREADS="1", MASTER_ADDR="127.0.0.1"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert open(out).read().strip() == "same bits", open(out).read()


def _pcg_longdouble(A, b, iters, tol=0.0):
    A = A.astype(np.longdouble)
    b = b.astype(np.longdouble)
    dinv = 1 / np.diag(A)
    x = np.zeros_like(b)
    r = b.copy()
    z = dinv * r
    p = z.copy()
    rho = r @ z
    for k in range(iters):
        Ap = A @ p
        alpha = rho / (p @ Ap)
        x += alpha * p
        r -= alpha * Ap
        if np.sqrt(r @ r) < tol:
            return x.astype(np.float64), k
        z = dinv * r
        rn = r @ z
        p = z + (rn / rho) * p
        rho = rn
    return x.astype(np.float64), iters


@pytest.mark.parametrize("p", [1, 3])
def test_jacobi_nonuniform_diagonal_against_longdouble(gpu_pkg, oracle, p):
    n = 1024
    L = oracle.generate_lap2d(n)
    sc = np.geomspace(1.0, 100.0, n)[np.random.default_rng(20261015).permutation(n)]
    A = (sc[:, None] * L) * sc[None, :]
    b = oracle.init_source_term(n)
    tol = 1e-6 * float(np.linalg.norm(b))
    xr, kref = _pcg_longdouble(A, b, 4 * n, tol)
    with solver(gpu_pkg, p) as s:
        s.set_matrix_csr(*dense_to_csr(A))
        s.set_preconditioner("jacobi")
        x, r = solve(s, n, 4 * n, tol)
    assert r["converged"] and abs(r["iterations"] - kref) <= 2
    assert np.linalg.norm(x - xr) / np.linalg.norm(xr) < 1e-6


@pytest.mark.parametrize("p", [1, 3])
def test_jacobi_missing_diagonal_is_refused(gpu_pkg, p):
    n = 300
    ip, ix, dv = lap2d_csr(n)
    rows = np.repeat(np.arange(n), np.diff(ip))
    keep = ~((rows == 123) & (ix == 123))                 # drop the entry (123, 123)
    assert keep.sum() == len(ix) - 1
    ip2 = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=n))])
    with solver(gpu_pkg, p) as s:
        s.set_matrix_csr(ip2, ix[keep], dv[keep])
        s.set_preconditioner("jacobi")
        with pytest.raises(gpu_pkg.CgxError) as e:
            solve(s, n, 20)
        assert e.value.status == BAD_ARG and "row 123" in str(e.value)
        s.set_preconditioner(None)                       # the context stays usable
        x, r = solve(s, n, 20, 0.0)
        assert r["iterations"] == 20


# ---- 7. refusals and plan -----------------------------------------------------------------------------------------------
def test_refusals(gpu_pkg):
    n = 2048
    with solver(gpu_pkg) as s:
        s.generate_lap2d_matrix(n)
        with pytest.raises(gpu_pkg.CgxError) as e:
            s.solve_multi(np.ones((2, n)))
        assert e.value.status == UNSUPPORTED
        with pytest.raises(gpu_pkg.CgxError) as e:
            s.probe_gemv_multi(np.ones((2, n)))
        assert e.value.status == UNSUPPORTED
        with pytest.raises(gpu_pkg.CgxError) as e:
            s.probe_fill_matrix_hash(1, symmetric=True, diag=4.0)
        assert e.value.status == UNSUPPORTED
    for variant in (40000, 50000, 10821, 30001, 70003, 70128):
        with solver(gpu_pkg, gemv_variant=variant) as s:
            with pytest.raises(gpu_pkg.CgxError) as e:
                s.generate_lap2d_matrix(n)
            assert e.value.status == UNSUPPORTED, variant


@pytest.mark.parametrize("variant", [0, -1])
def test_default_plan_is_variant_7_never_persistent(gpu_pkg, variant):
    n = 2048
    with solver(gpu_pkg, gemv_variant=variant) as s:
        s.generate_lap2d_matrix(n)
        plan = s.gemv_plan()
        assert plan["variant"] == 7 and plan["grid"] == 32 and plan["waves"] == 4
        x, r = solve(s, n, 50)
        assert s.resident_record()["persistent"] == 0


# ---- 8. CLI and the RCCL transport --------------------------------------------------------------------------------------
def _step(stdout):
    return int([ln for ln in stdout.splitlines() if "[STEP" in ln][0].split("[STEP")[1].split("]")[0])


def test_cli_csr_agrees_with_banded(gpu_pkg, mtx_path, tmp_path):
    out = tmp_path / "out.txt"
    for args in (["4096", str(out)], [mtx_path, str(out)]):
        k = {}
        for flag in ("--banded", "--csr"):
            r = subprocess.run([EXE] + args + [flag, "--stats"], capture_output=True, text=True, timeout=300)
            assert r.returncode == 0, r.stderr
            k[flag] = _step(r.stdout)
            if flag == "--csr":
                assert re.search(r"format=csr nnz=\d+", r.stderr), r.stderr[-2000:]
        assert abs(k["--csr"] - k["--banded"]) <= 0.1 * k["--banded"], k


def _loop_bodies(stderr):
    m = re.search(r"cgsolver stats: .*", stderr)
    assert m, stderr[-2000:]
    return m.group(0), int(re.search(r"loop_bodies=(\d+)", m.group(0)).group(1))


@pytest.fixture(scope="module")
def fake_rccl_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("fake_rccl_csr")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-w", "-O2", "-std=c++17", "-fPIC", "-shared", "-I/opt/rocm/include",
                           os.path.join(ROOT, "tests", "fake_rccl", "fake_rccl.cc"), "-o", str(d / "librccl.so.1"),
                           "-Wl,-soname,librccl.so.1"], timeout=600)
    return str(d)


def test_cli_rccl_transport(gpu_pkg, fake_rccl_dir, tmp_path):
    env = dict(os.environ, LD_LIBRARY_PATH=fake_rccl_dir + os.pathsep + os.environ.get("LD_LIBRARY_PATH", ""))
    base = ["2048", str(tmp_path / "out"), "--gpus", "2", "--same-device", "--transport", "rccl", "--stats"]
    runs = {}
    for name, extra in (("banded", ["--banded"]), ("csr", ["--csr"]), ("csr_jacobi", ["--csr", "--jacobi"]), ("jacobi", ["--jacobi"])):
        r = subprocess.run([EXE] + base + extra, capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0, (name, r.stderr[-2000:])
        runs[name] = _loop_bodies(r.stderr)
    assert "format=csr nnz=" in runs["csr"][0]
    assert abs(runs["csr"][1] - runs["banded"][1]) <= 1
    assert abs(runs["csr_jacobi"][1] - runs["jacobi"][1]) <= 1
    assert runs["csr_jacobi"][0].endswith("precond=jacobi")
