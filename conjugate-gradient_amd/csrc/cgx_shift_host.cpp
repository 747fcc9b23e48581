// cgx_shift_host.cpp -- cgx_solve_shifted: the host side of multi-shift CG (cgx_shift.hip).
//
// One GPU, dense or CSR storage.  The seed runs in the single path's own buffers with the single path's own loop body
// (enqueue_iteration, cgx_solve.cpp): whatever per-launch K1 the shard's plan names, K3 behind it, and behind K3 the shift kernel.
// Where the context's plan is a persistent kernel nothing of it is touched: the loop below never asks for it, and the next
// cgx_solve_begin sets the state up again from scratch.  The x and p of the shifts, the block of the final verification and the
// shift scalars live in ONE device allocation of the context (cgx_ctx::shift), made on first use and freed with the problem.
#include "cgx_internal.h"

using namespace cgxi;

namespace {

constexpr int kS = cgx::kMaxShifts;

struct ShiftView {
    double *X, *P, *Y;          // kS x lda each (shift j at + j * lda)
    double *k1p;                // dense verification: the multi-vector K1's p.Ap partials (written, never read)
    cgx::MultiScalars *ms;      // ... and its scalar block (the plain form does not touch it)
    cgx::ShiftScalars *ss;
};

size_t shift_layout(const cgx_ctx *ctx, double *base, ShiftView *v)
{
    const size_t vec = (size_t)kS * ctx->lda;
    Carver c{base};
    v->X = c.take(vec);
    v->P = c.take(vec);
    v->Y = c.take(vec);
    v->k1p = c.take((size_t)kS * k1p_stride(ctx->n));
    v->ms = c.take_struct<cgx::MultiScalars>();
    v->ss = c.take_struct<cgx::ShiftScalars>();
    return c.bytes();
}

// The context's shift block, made on first use.
cgx_status ensure_shift(cgx_ctx *ctx, ShiftView *v)
{
    CGX_TRY(ensure_side_block(ctx, &ctx->shift, &ctx->shift_bytes, shift_layout(ctx, nullptr, v)));
    shift_layout(ctx, ctx->shift, v);
    return CGX_OK;
}

}  // namespace

extern "C" {

cgx_status cgx_solve_shifted(cgx_ctx *ctx, int nshift, const double *sigma, double *X, long ldx, cgx_result *res)
{
    CGX_TRY(check_shift_call(ctx, "cgx_solve_shifted", "CGX_MAX_SHIFTS", false,
                             "no preconditioner (it breaks the collinearity of the shifted residuals; cgx_set_preconditioner)", "shifted",
                             nshift, sigma, X, ldx));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    ShiftView v;
    CGX_TRY(ensure_shift(ctx, &v));
    Shard &s = ctx->shards[0];
    hipStream_t st = ctx->stream;
    const int n = ctx->n;
    const long lda = ctx->lda;
    reset_gemv_stats(ctx);
    const double t_begin = wall_now();

    // The seed's set-up: cgx_solve_begin (cg.cc:49-92) for x0 = 0 without its GEMV -- A 0 is exactly 0, so r0 = b - 0 = b, and
    // launch_init_residual on zeroed segments leaves r and the r.r partials of iteration 0's head as that begin leaves them.
    HIP_TRY(ctx, hipMemsetAsync(s.sc, 0, sizeof(Scalars), st));
    HIP_TRY(ctx, hipMemsetAsync(s.apg, 0, (size_t)ctx->nranks * ctx->seg_S * sizeof(double), st));
    HIP_TRY(ctx, hipMemsetAsync(s.rbuf, 0, (size_t)s.rv.S * sizeof(double), st));
    HIP_TRY(ctx, hipMemsetAsync(s.x, 0, (size_t)s.rows * sizeof(double), st));
    HIP_TRY(ctx, hipMemsetAsync(s.p[0], 0, (size_t)lda * sizeof(double), st));
    HIP_TRY(ctx, hipMemsetAsync(s.p[1], 0, (size_t)lda * sizeof(double), st));
    HIP_TRY(ctx, cgx::launch_init_residual(n, s.b_full, s.apv, s.rv, s.partials, st));
    HIP_TRY(ctx, cgx::launch_shift_begin(n, lda, nshift, sigma, s.b_full, v.X, v.P, v.ss, st));

    cgx::ShiftArgs a{};
    a.n = n;
    a.nshift = nshift;
    a.lda = lda;
    a.r = s.rv.base;
    a.rrp = s.rv.base + s.rv.Sr;
    a.nrr = s.rv.S - s.rv.Sr;
    // the p.Ap partials exactly as enqueue_iteration hands them to K3 on one GPU: at the head of the tail; variant 6 leaves one
    // per fold workgroup, every other plan ctx->npart (K1's workgroups, or, column pieces added up first, the chunks of the slice)
    a.pap = s.apg + s.apv.Sr;
    a.npap = s.plan.variant == 6 ? cgx::plan_partials(s.plan) : ctx->npart;
    a.pap_strided = (long)cgx::update_xr_grid(n) * 256 >= n ? 0 : 1;
    a.sc = s.sc;
    a.ss = v.ss;
    a.X = v.X;
    a.P = v.P;
    a.tol = ctx->tol;

    // the loop cg.cc:95-137 as cgx_solve_steps runs it: the seed's done flag -- raised by the seed's own head or by the shift kernel
    // that found every shift frozen -- is polled every check_every iterations, one batch kept queued
    const double t0 = wall_now();
    auto iteration = [&](int i) -> cgx_status {
        CGX_TRY(enqueue_iteration(ctx, i));
        a.k = i;
        HIP_TRY(ctx, cgx::launch_shift_update(a, st));
        return CGX_OK;
    };
    int k = 0;
    CGX_TRY(run_polled(ctx, &s.sc->done, ctx->max_iter, ctx->cfg.profile_gemv && ctx->max_iter > 0, iteration, &k));
    HIP_TRY(ctx, cgx::launch_shift_close(v.ss, a.rrp, a.nrr, nshift, k, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    const double t_loop = wall_now() - t0;

    // always the full width kS: a row's sum order depends on the kernel width, and a shift's result must not depend on how many
    // others there are (the columns beyond nshift hold zeros or an earlier call's x)
    CGX_TRY(column_residual_norms(ctx, nshift, kS, v.X, v.Y, v.k1p, v.ms, s.b_full, 0, sigma, &v.ss->norms[0][0]));
    cgx::ShiftScalars hs;
    HIP_TRY(ctx, hipMemcpyAsync(&hs, v.ss, sizeof hs, hipMemcpyDeviceToHost, st));
    CGX_TRY(download_columns(ctx, X, ldx, v.X, nshift));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    if (ctx->ev_used || ctx->upd_used || ctx->steps_ev_pending) CGX_TRY(harvest_gemv_events(ctx));

    fill_column_results(ctx, res, nshift, t_begin, t_loop, one_gpu_gemv_bytes(ctx), true, hs.norms, [&](int j) {
        const bool frozen = hs.frozen_at[j] != cgx::kShiftLive;
        return ColumnOutcome{frozen ? hs.frozen_at[j] : k, frozen ? 1 : 0, hs.res_prev[j], hs.res_last[j]};
    });
    return CGX_OK;
}

}  // extern "C"
