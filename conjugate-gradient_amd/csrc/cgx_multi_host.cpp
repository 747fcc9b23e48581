// cgx_multi_host.cpp -- cgx_solve_multi, cgx_solve_multi_pc and cgx_probe_gemv_multi: the host side of the multi-vector kernels
// (cgx_multi.hip; with a preconditioner cgx_multi_pc.hip).
//
// One GPU, dense storage.  The k-wide blocks live in ONE device allocation of the context (cgx_ctx::multi), apart from the single
// path's per-shard buffers and state blocks, so that a multi solve changes nothing a single solve reads: neither the plan, nor
// x / r / p, nor the scalar block.  It is made on the first multi call of a problem and freed with the problem.  What the
// preconditioned call needs on top (Z, the r.z partials, the partials of L^T r, r.r's scalars) is a second block of the same kind
// (cgx_ctx::multi_pc), so the first keeps its layout.  The preconditioner itself -- the inverse diagonal, or L, C^-1 and delta -- is
// the single path's, made by prepare_jacobi / prepare_lowrank once per matrix and shared in both directions.
#include "cgx_internal.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

using namespace cgxi;

namespace {

constexpr int kW = cgx::kMaxRhs;

struct MultiView {
    double *B, *X, *R, *P[2], *Y;   // kW x lda each (column j at + j * lda)
    double *k1p;                    // kW x multi_gemv_grid(n, 1): K1m's p.Ap partials (grid of the widest-row shape at most)
    double *rrp;                    // kW x multi_update_grid(n): K3m's r.r partials
    cgx::MultiScalars *ms;
};

size_t multi_layout(const cgx_ctx *ctx, double *base, MultiView *v)
{
    const size_t vec = (size_t)kW * ctx->lda;
    Carver c{base};
    v->B = c.take(vec);
    v->X = c.take(vec);
    v->R = c.take(vec);
    v->P[0] = c.take(vec);
    v->P[1] = c.take(vec);
    v->Y = c.take(vec);
    v->k1p = c.take((size_t)kW * k1p_stride(ctx->n));
    v->rrp = c.take((size_t)kW * cgx::multi_update_grid(ctx->n));
    v->ms = c.take_struct<cgx::MultiScalars>();
    return c.bytes();
}

// The preconditioned call's own block.
struct PcView {
    double *Z;                      // kW x lda
    double *rzp;                    // kW x multi_update_grid(n): the r.z partials
    double *tpart;                  // kW x lr_grid(n) x kLrLd: the partials of t_j = L^T r_j (pivoted Cholesky)
    cgx::MultiPcScalars *mp;
};

size_t pc_layout(const cgx_ctx *ctx, double *base, PcView *v)
{
    Carver c{base};
    v->Z = c.take((size_t)kW * ctx->lda);
    v->rzp = c.take((size_t)kW * cgx::multi_update_grid(ctx->n));
    v->tpart = c.take((size_t)kW * cgx::multi_update_grid(ctx->n) * cgx::kLrLd);
    v->mp = c.take_struct<cgx::MultiPcScalars>();
    return c.bytes();
}

// The checks every multi entry point makes, in this order: context, problem, transport and storage, arguments.
cgx_status check_multi(cgx_ctx *ctx, const char *name, int nrhs, const void *in, long ldin, const void *out, long ldout)
{
    const std::string fn(name);
    CGX_TRY(check_dense_one_gpu(ctx, fn));
    if (nrhs < 1 || nrhs > CGX_MAX_RHS) return fail(ctx, CGX_ERR_BAD_ARG, fn + ": nrhs must be 1 .. CGX_MAX_RHS");
    if (!in || !out) return fail(ctx, CGX_ERR_BAD_ARG, fn + ": null pointer");
    if (ldin < ctx->n || ldout < ctx->n) return fail(ctx, CGX_ERR_BAD_ARG, fn + ": leading dimension smaller than n");
    return CGX_OK;
}

// The context's multi block, made on first use.
cgx_status ensure_multi(cgx_ctx *ctx, MultiView *v)
{
    CGX_TRY(ensure_side_block(ctx, &ctx->multi, &ctx->multi_bytes, multi_layout(ctx, nullptr, v)));
    multi_layout(ctx, ctx->multi, v);
    return CGX_OK;
}

cgx_status ensure_multi_pc(cgx_ctx *ctx, PcView *v)
{
    CGX_TRY(ensure_side_block(ctx, &ctx->multi_pc, &ctx->multi_pc_bytes, pc_layout(ctx, nullptr, v)));
    pc_layout(ctx, ctx->multi_pc, v);
    return CGX_OK;
}

// What the preconditioned kernels take, for the context's kind (behind prepare_jacobi / prepare_lowrank).
cgx::MultiPcArgs pc_args(const cgx_ctx *ctx, const PcView &pv)
{
    cgx::MultiPcArgs a{};
    a.Z = pv.Z;
    a.rzp = pv.rzp;
    a.mp = pv.mp;
    a.M = pc_factor(ctx, pv.tpart);
    return a;
}

cgx::MultiArgs plain_args(cgx_ctx *ctx, const MultiView &v, int nrhs, const double *vec)
{
    cgx::MultiArgs g = plain_k1m_args(ctx, nrhs, vec, v.Y, v.k1p);
    g.ms = v.ms;
    return g;
}

// K1m fused of iteration k, event-timed where next_gemv_events says so (as run_gemv_fused, cgx_solve.cpp); pc: the preconditioned
// head, p = z + beta p_old
cgx_status run_multi_fused(cgx_ctx *ctx, const MultiView &v, int nrhs, int k, const cgx::MultiPcArgs *pc)
{
    hipEvent_t e0, e1;
    CGX_TRY(next_gemv_events(ctx, &e0, &e1));
    cgx::MultiArgs g = plain_args(ctx, v, nrhs, v.P[k & 1]);
    g.p_new = v.P[(k + 1) & 1];
    g.r = pc ? pc->Z : v.R;
    g.rrp = v.rrp;
    g.k = k;
    g.tol = ctx->tol;
    if (pc) HIP_TRY(ctx, cgx::launch_multi_gemv_pc(g, *pc, ctx->stream, e0, e1));
    else HIP_TRY(ctx, cgx::launch_multi_gemv(g, true, ctx->stream, e0, e1));
    return CGX_OK;
}

// THE multi solve: set-up, the polled loop, the final product and the results.  pre: every column runs the recurrence of DESIGN.md
// section 11 with the context's preconditioner (already prepared); otherwise the plain one.  The preconditioner is the varying
// part: which K1m head, which K3m, the launch behind the initial residual, which r.r the results read.
cgx_status solve_multi_body(cgx_ctx *ctx, bool pre, int nrhs, const double *B, long ldb, double *X, long ldx, cgx_result *res)
{
    MultiView v;
    CGX_TRY(ensure_multi(ctx, &v));
    PcView pv{};
    cgx::MultiPcArgs pc{};
    if (pre) {
        CGX_TRY(ensure_multi_pc(ctx, &pv));
        pc = pc_args(ctx, pv);
    }
    hipStream_t st = ctx->stream;
    const int n = ctx->n;
    const long lda = ctx->lda;
    const int g1 = cgx::multi_gemv_grid(n, cgx::multi_width(nrhs));
    reset_gemv_stats(ctx);
    const double t_begin = wall_now();

    // set-up, cg.cc:49-92 per column: r = b - A x0, p_old = 0, the r.r partials of iteration 0's head (pre: z0 and its partials)
    CGX_TRY(upload_columns(ctx, v.B, B, ldb, nrhs));
    CGX_TRY(upload_columns(ctx, v.X, X, ldx, nrhs));
    HIP_TRY(ctx, hipMemsetAsync(v.ms, 0, sizeof(cgx::MultiScalars), st));
    if (pre) HIP_TRY(ctx, hipMemsetAsync(pv.mp, 0, sizeof(cgx::MultiPcScalars), st));
    HIP_TRY(ctx, hipMemsetAsync(v.P[0], 0, (size_t)nrhs * lda * sizeof(double), st));
    HIP_TRY(ctx, cgx::launch_multi_gemv(plain_args(ctx, v, nrhs, v.X), false, st));
    HIP_TRY(ctx, cgx::launch_multi_init(n, lda, nrhs, v.B, v.Y, v.R, v.rrp, st));
    if (pre) HIP_TRY(ctx, cgx::launch_multi_update_pc(n, lda, nrhs, nullptr, nullptr, nullptr, 0, nullptr, v.R, v.rrp, v.ms, 0, pc, true, st));

    // the loop cg.cc:95-137: K1m + K3m per iteration; all_done is polled every check_every iterations, one batch kept queued
    const double t0 = wall_now();
    auto iteration = [&](int i) -> cgx_status {
        CGX_TRY(run_multi_fused(ctx, v, nrhs, i, pre ? &pc : nullptr));
        if (pre)
            HIP_TRY(ctx, cgx::launch_multi_update_pc(n, lda, nrhs, v.P[(i + 1) & 1], v.Y, v.k1p, g1, v.X, v.R, v.rrp, v.ms, i & 1, pc, false, st));
        else
            HIP_TRY(ctx, cgx::launch_multi_update(n, lda, nrhs, v.P[(i + 1) & 1], v.Y, v.k1p, g1, v.X, v.R, v.rrp, v.ms, i & 1, st));
        return CGX_OK;
    };
    int k = 0;
    CGX_TRY(run_polled(ctx, &v.ms->all_done, ctx->max_iter, false, iteration, &k));   // (no device-side window: steps_device_ms stays 0)
    // the head of iteration k for the columns still running (cg.cc:117-121,132), then x and the DEBUG norms (cg.cc:140-151)
    if (pre) HIP_TRY(ctx, cgx::launch_multi_close_pc(v.ms, pc, v.rrp, n, nrhs, k, ctx->tol, st));
    else HIP_TRY(ctx, cgx::launch_multi_close(v.ms, v.rrp, n, nrhs, k, ctx->tol, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    const double t_loop = wall_now() - t0;
    CGX_TRY(column_residual_norms(ctx, nrhs, nrhs, v.X, v.Y, v.k1p, v.ms, v.B, lda, nullptr, &v.ms->norms[0][0]));
    cgx::MultiScalars hs;
    cgx::MultiPcScalars hp;
    HIP_TRY(ctx, hipMemcpyAsync(&hs, v.ms, sizeof hs, hipMemcpyDeviceToHost, st));
    if (pre) HIP_TRY(ctx, hipMemcpyAsync(&hp, pv.mp, sizeof hp, hipMemcpyDeviceToHost, st));
    CGX_TRY(download_columns(ctx, X, ldx, v.X, nrhs));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    if (ctx->ev_used || ctx->upd_used || ctx->steps_ev_pending) CGX_TRY(harvest_gemv_events(ctx));

    fill_column_results(ctx, res, nrhs, t_begin, t_loop, 8.0 * ((double)n * n + 2.0 * nrhs * n), true, hs.norms, [&](int j) {
        const bool done = hs.done[j] != 0;
        const int k_exit = done ? hs.k_final[j] : k;
        const double *rr = pre ? hp.rr[j] : hs.rs[j];                   // pre: rs[] holds r.z, the report is sqrt(r.r)
        const double prev = std::sqrt(rr[k_exit & 1]);                  // sqrt(rsold) as printed, cg.cc:152-153
        return ColumnOutcome{k_exit, done ? 1 : 0, prev, done ? std::sqrt(rr[(k_exit + 1) & 1]) : prev};
    });
    return CGX_OK;
}

}  // namespace

extern "C" {

cgx_status cgx_solve_multi(cgx_ctx *ctx, int nrhs, const double *B, long ldb, double *X, long ldx, cgx_result *res)
{
    CGX_TRY(check_multi(ctx, "cgx_solve_multi", nrhs, B, ldb, X, ldx));
    if (ctx->precond != CGX_PRECOND_NONE)
        return fail(ctx, CGX_ERR_UNSUPPORTED, "cgx_solve_multi: no preconditioner for several right-hand sides (cgx_set_preconditioner)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return solve_multi_body(ctx, false, nrhs, B, ldb, X, ldx, res);
}

cgx_status cgx_solve_multi_pc(cgx_ctx *ctx, int nrhs, const double *B, long ldb, double *X, long ldx, cgx_result *res)
{
    CGX_TRY(check_multi(ctx, "cgx_solve_multi_pc", nrhs, B, ldb, X, ldx));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const bool pre = ctx->precond != CGX_PRECOND_NONE;
    if (pre) CGX_TRY(prepare_multi_precond(ctx, "cgx_solve_multi_pc"));
    return solve_multi_body(ctx, pre, nrhs, B, ldb, X, ldx, res);
}

// TEST PROBE: Z_j = M^-1 R_j for nrhs caller's vectors (one per row) through the preconditioned multi path's own kernels, the
// set-up form of K3m (Jacobi: one launch; pivoted Cholesky: update + apply).  Needs a preconditioner; prepares it like a solve.
cgx_status cgx_probe_multi_pc_apply(cgx_ctx *ctx, int nrhs, const double *R, long ldr, double *Z, long ldz)
{
    CGX_TRY(check_multi(ctx, "cgx_probe_multi_pc_apply", nrhs, R, ldr, Z, ldz));
    if (ctx->precond == CGX_PRECOND_NONE) return fail(ctx, CGX_ERR_BAD_ARG, "cgx_probe_multi_pc_apply: no preconditioner is set");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    CGX_TRY(prepare_multi_precond(ctx, "cgx_probe_multi_pc_apply"));
    MultiView v;
    PcView pv{};
    CGX_TRY(ensure_multi(ctx, &v));
    CGX_TRY(ensure_multi_pc(ctx, &pv));
    const cgx::MultiPcArgs pc = pc_args(ctx, pv);
    CGX_TRY(upload_columns(ctx, v.R, R, ldr, nrhs));
    HIP_TRY(ctx, cgx::launch_multi_update_pc(ctx->n, ctx->lda, nrhs, nullptr, nullptr, nullptr, 0, nullptr, v.R, v.rrp, v.ms, 0, pc, true,
                                             ctx->stream));
    CGX_TRY(download_columns(ctx, Z, ldz, pv.Z, nrhs));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return CGX_OK;
}

cgx_status cgx_probe_gemv_multi(cgx_ctx *ctx, int nrhs, const double *P, long ldp, double *Y, long ldy, double *pAp)
{
    CGX_TRY(check_multi(ctx, "cgx_probe_gemv_multi", nrhs, P, ldp, Y, ldy));
    if (!pAp) return fail(ctx, CGX_ERR_BAD_ARG, "cgx_probe_gemv_multi: null pointer");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    MultiView v;
    CGX_TRY(ensure_multi(ctx, &v));
    const int g1 = cgx::multi_gemv_grid(ctx->n, cgx::multi_width(nrhs));
    CGX_TRY(upload_columns(ctx, v.P[0], P, ldp, nrhs));
    HIP_TRY(ctx, cgx::launch_multi_gemv(plain_args(ctx, v, nrhs, v.P[0]), false, ctx->stream));
    std::vector<double> parts((size_t)nrhs * g1);
    HIP_TRY(ctx, hipMemcpyAsync(parts.data(), v.k1p, parts.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    CGX_TRY(download_columns(ctx, Y, ldy, v.Y, nrhs));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (int j = 0; j < nrhs; ++j) {   // the workgroups' partials in ascending order
        double s = 0.0;
        for (int g = 0; g < g1; ++g) s += parts[(size_t)j * g1 + g];
        pAp[j] = s;
    }
    return CGX_OK;
}

}  // extern "C"
