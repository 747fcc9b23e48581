"""Build-time and host-only checks of the preconditioned Lanczos quadrature entry points (cgx_lanczos_pc, cgx_precond_logdet,
cgx_slq_probes, cgx_trace_slq_pc): the symbols, their prototypes and the Python methods, argument checks
without a context, the float64 restatement against the longdouble one, the register report of every kernel in
csrc/cgx_lanczos_pc.hip, and the argument errors of cgsolver --logdet-pc."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import lanczos_pc_reference as pref
import lanczos_reference as ref
import pivchol_reference
from test_lanczos_abi import _resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
DP = C.POINTER(C.c_double)


def _dp(a):
    return a.ctypes.data_as(DP)


def test_symbols_and_prototypes(pkg):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cgx.h")).read(), flags=re.S)
    flat = re.sub(r"\s+", " ", text)
    for proto in (
        "cgx_status cgx_lanczos_pc(cgx_ctx *ctx, int nvec, int steps, const double *V0, long ldv, double *alpha, double *beta, "
        "int *steps_done, double *eta2);",
        "cgx_status cgx_precond_logdet(cgx_ctx *ctx, double *logdet);",
        "cgx_status cgx_slq_probes(cgx_ctx *ctx, int fn, int nprobe, unsigned long long seed, double *Z, long ldz);",
        "cgx_status cgx_trace_slq_pc(cgx_ctx *ctx, int fn, int nprobe, int steps, unsigned long long seed, const double *Z, long ldz, "
        "double *estimate, double *std_error, double *per_probe, double *ritz, double *logdet_precond);",
    ):
        assert proto in flat, proto
    cgx = pkg.cgx
    out = subprocess.run(["nm", "-D", "--defined-only", cgx.LIB_PATH], capture_output=True, text=True).stdout
    for name in ("cgx_lanczos_pc", "cgx_precond_logdet", "cgx_slq_probes", "cgx_trace_slq_pc"):
        assert name in cgx.EXPORTS and re.search(r" T %s\b" % name, out), name
    for name in ("lanczos_pc", "precond_logdet", "slq_probes", "logdet_pc", "trace_inv_pc"):
        assert hasattr(pkg.CGSolver, name), name
    # the header says who answers for the covariance of caller probes
    doc = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "cgx.h")).read())
    assert "CALLER ANSWERS FOR THE COVARIANCE" in doc


def test_null_context_is_bad_arg(pkg):
    L = pkg.cgx.lib()
    v = np.ones(8)
    a, b, e2 = np.zeros(4), np.zeros(4), np.zeros(1)
    done = (C.c_int * 1)()
    est, err, ldm = C.c_double(), C.c_double(), C.c_double()
    assert L.cgx_lanczos_pc(None, 1, 4, _dp(v), 8, _dp(a), _dp(b), done, _dp(e2)) == 1
    assert L.cgx_precond_logdet(None, C.byref(ldm)) == 1
    assert L.cgx_slq_probes(None, 0, 1, 1, _dp(v), 8) == 1
    assert L.cgx_trace_slq_pc(None, 0, 1, 4, 1, None, 0, C.byref(est), C.byref(err), None, None, None) == 1


def _kernel_case(n, rank):
    A, _ = pivchol_reference.kernel_matrix(n, 0.2, 1e-2)
    _, L, delta, _ = pivchol_reference.pivoted_cholesky(A, rank)
    return A, L, delta


def test_restatement_matches_the_high_precision_reference():
    """tests/lanczos_pc_reference.py against itself: over 12 steps the float64 recurrence stays within the floor of the tolerance
    rule (relative to max |alpha|) of the longdouble one with full reorthogonalisation in the M-inner product, under the pivoted-
    Cholesky factor of a kernel matrix and under Jacobi; eta0^2 agrees; T is the Jacobi matrix of M^-1/2 A M^-1/2."""
    n, rank, steps = 257, 16, 12
    A, L, delta = _kernel_case(n, rank)
    v0 = np.random.default_rng(5).standard_normal(n)
    for name, ap64, apld in (("pivchol", pref.lowrank_apply(L, delta), pref.lowrank_apply(L, delta, pref.LD)),
                             ("jacobi", pref.jacobi_apply(A), pref.jacobi_apply(A, pref.LD))):
        a, b, m, e2 = pref.lanczos_pc_f64(A, ap64, v0, steps)
        al, bl, e2l = pref.lanczos_pc_longdouble(A, apld, v0, steps)
        assert m == steps
        scale = float(np.max(np.abs(al)))
        dev = float(max(np.max(np.abs(a - al)), np.max(np.abs(b - bl)))) / scale
        print("%s: restatement against longdouble over %d steps: %.3e (floor %.3e)" % (name, steps, dev, ref.tolerance(0.0, n)))
        assert dev <= ref.tolerance(0.0, n), (name, dev)
        assert abs(e2 - float(e2l)) <= ref.tolerance(0.0, n) * float(e2l)
    # (alpha, beta) are the Jacobi matrix of B = G^-1 A G^-T from g = G^-1 v0 (M = G G^T): a 12-point Gauss rule is exact for the
    # moments g^T B^p g, p <= 23.  Checked for p = 0 .. 3 against the dense B, whose float64 formation through the explicit inverse
    # of G carries a relative error of about cond(M) 2^-52; the bound gives it, the products and the rule 64 times that.
    M = L @ L.T + delta * np.eye(n)
    Gi = np.linalg.inv(np.linalg.cholesky(M))
    B = Gi @ A @ Gi.T
    g = Gi @ v0
    bound = 64 * float(np.linalg.cond(M)) * ref.EPS
    a, b, m, e2 = pref.lanczos_pc_f64(A, pref.lowrank_apply(L, delta), v0, steps)
    x = g.copy()
    for p in range(4):
        exact = float(g @ x)
        got = ref.quadrature(a, b, m, e2, lambda th: th ** p)
        print("moment %d: rule %.15e dense %.15e, relative %.2e (bound %.2e)" % (p, got, exact, abs(got - exact) / abs(exact), bound))
        assert abs(got - exact) <= bound * abs(exact), (p, got, exact)
        x = B @ x


def test_restatement_finds_the_invariant_subspace():
    """The breakdown matrix under Jacobi: D^-1/2 A D^-1/2 has four distinct eigenvalues, so a Rademacher-type start stops with m = 4
    and the start sqrt(d) v2 with m = 1; the quadratures are g^T log(B / B_00) g."""
    A, s, vec, c, b00 = pref.breakdown_matrix(1000)
    ap = pref.jacobi_apply(A)
    Z = pref.probes_log_jacobi(1, 8, A)
    assert np.all(ref.rademacher(1, 8, 1000) @ vec.T != 0)    # seed 1: every probe has a part in each of the three directions
    for j in range(8):
        a, b, m, e2 = pref.lanczos_pc_f64(A, ap, Z[j], 12)
        amax = np.max(np.abs(a))
        # the decision is far from its threshold on both sides: the other betas lie above 2^-18 max |alpha|, its square root
        assert m == 4 and b[3] <= ref.BREAK * amax and np.all(b[:3] >= 2.0 ** -18 * amax), (j, m, b)
        assert np.all(a[4:] == 0) and np.all(b[4:] == 0)
        g = Z[j] / np.sqrt(np.diag(A))
        terms = pref.breakdown_log_terms(g, vec, c)
        exact, scale = float(terms.sum()), float(np.abs(terms).sum())
        assert abs(ref.quadrature(a, b, m, e2, np.log) - exact) <= ref.tolerance(0.0, 1000) * scale, j
    a, b, m, e2 = pref.lanczos_pc_f64(A, ap, np.sqrt(np.diag(A)) * vec[1], 12)
    assert m == 1 and abs(a[0] - 8.0 / b00) <= 1e-13


def test_probe_restatement_has_the_preconditioners_covariance():
    """z = L g + sqrt(delta) s: over the 2^(n + k) sign patterns E[z z^T] = L L^T + delta I.  Checked on the structure: the probe is
    linear in the signs with the matrix [sqrt(delta) I | L]."""
    n, rank = 64, 5
    A, L, delta = _kernel_case(n, rank)
    Z = pref.probes_log_lowrank(9, 4, L, delta)
    S = ref.rademacher(9, 4, n + rank)
    W = np.hstack([np.sqrt(delta) * np.eye(n), L])
    assert np.max(np.abs(Z - S @ W.T)) <= (rank + 2) * 2.0 ** -53 * float(np.max(np.sum(np.abs(W), axis=1)))
    assert np.max(np.abs(W @ W.T - (L @ L.T + delta * np.eye(n)))) <= 1e-14 * float(np.max(np.abs(L @ L.T)))
    assert np.array_equal(pref.probes_log_jacobi(9, 4, A), ref.rademacher(9, 4, n) * np.sqrt(np.diag(A)))


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_lanczos_pc_kernels_never_spill():
    rows = [r for r in _resources("cgx_lanczos_pc.hip") if "cgx::" in r["name"]]
    names = sorted(re.search(r"(k_lpc_\w+)", r["name"]).group(1) for r in rows)
    want = ["k_lpc_begin", "k_lpc_close", "k_lpc_jac_step", "k_lpc_jac_step", "k_lpc_lr_apply", "k_lpc_lr_apply", "k_lpc_lr_apply",
            "k_lpc_lr_apply", "k_lpc_lr_apply", "k_lpc_lr_step", "k_lpc_lr_step", "k_lpc_probes"]
    assert names == want, [r["name"] for r in rows]
    for r in rows:
        assert int(r["VGPRs Spill"]) == 0 and int(r["ScratchSize [bytes/lane]"]) == 0, r
        assert int(r.get("SGPRs Spill", "0")) == 0, r


def test_cli_logdet_pc_argument_checks(pkg, tmp_path):
    exe = os.path.join(ROOT, "conjugate-gradient_amd", "cgsolver")
    out = str(tmp_path / "never_written.txt")
    for args, needle in ((["--logdet-pc", "8"], "needs a preconditioner"),
                         (["--logdet-pc", "8", "--jacobi", "--shifts", "0,1"], "not together with --shifts"),
                         (["--logdet-pc", "0", "--jacobi"], "--logdet-pc takes"), (["--logdet-pc", "257", "--jacobi"], "--logdet-pc takes"),
                         (["--logdet-pc", "8,0", "--pivchol", "16"], "--logdet-pc takes"),
                         (["--logdet-pc", "8,x", "--pivchol", "16"], "--logdet-pc takes")):
        r = subprocess.run([exe, "64", out] + args, capture_output=True, text=True)
        assert r.returncode == 1 and needle in r.stderr and "Usage" in r.stderr, (args, r.stderr[:300])
        assert not os.path.exists(out)
    assert "--logdet-pc P[,M]" in subprocess.run([exe], capture_output=True, text=True).stderr
