// cgx_minres_host.cpp -- cgx_solve_minres: the host side of MINRES (cgx_minres.hip).
//
// One GPU, dense or CSR storage.  A launch is the plain K1 of the shard's plan (run_gemv_plain: general dense, the symmetric
// upper-triangle kernel, CSR) on the recurrence's own vector, then the step kernel; the product and its partials land where the
// plain K1 always leaves them (the shard's Ap slice and segment tail), which every solve sets up again from scratch.  Where the
// context's plan is a persistent kernel nothing of it is touched.  The x and the directions of the shifts, the block of the final
// verification, the recurrence vectors, the partials and the scalars live in ONE device allocation of the context
// (cgx_ctx::minres), made on first use and freed with the problem.
#include "cgx_internal.h"

using namespace cgxi;

namespace {

constexpr int kS = cgx::kMaxMinresShifts;

struct MinresView {
    double *X, *D[2], *Y;       // kS x lda each (shift j at + j * lda); Y: the verification's products
    double *V[2];               // lda each, zero padded (the plain K1 reads a full vector): w_t / v_(t-1), swapped between launches
    double *wwp[2];             // update_xr_grid(n) each: the ||w||^2 partials, ping-pong over the launches
    double *k1p;                // dense verification: the multi-vector K1's partials (written, never read)
    cgx::MultiScalars *vm;      // ... and its scalar block (the plain form does not touch it)
    double *norms;              // 3 x kS: what launch_column_norms leaves
    cgx::MinresScalars *ms;
};

size_t minres_layout(const cgx_ctx *ctx, double *base, MinresView *v)
{
    const size_t vec = (size_t)kS * ctx->lda, g3 = (size_t)cgx::update_xr_grid(ctx->n);
    Carver c{base};
    v->X = c.take(vec);
    v->D[0] = c.take(vec);
    v->D[1] = c.take(vec);
    v->Y = c.take(vec);
    v->V[0] = c.take((size_t)ctx->lda);
    v->V[1] = c.take((size_t)ctx->lda);
    v->wwp[0] = c.take(g3);
    v->wwp[1] = c.take(g3);
    v->k1p = c.take(ctx->csr ? 0 : (size_t)kS * k1p_stride(ctx->n));
    v->vm = c.take_struct<cgx::MultiScalars>();
    v->norms = c.take(3 * (size_t)kS);
    v->ms = c.take_struct<cgx::MinresScalars>();
    return c.bytes();
}

}  // namespace

extern "C" {

cgx_status cgx_solve_minres(cgx_ctx *ctx, int nshift, const double *sigma, double *X, long ldx, cgx_result *res)
{
    CGX_TRY(check_shift_call(ctx, "cgx_solve_minres", "CGX_MAX_MINRES_SHIFTS", true,
                             "a preconditioner is set and would be ignored (cgx_set_preconditioner)", "MINRES", nshift, sigma, X, ldx));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    MinresView v;
    CGX_TRY(ensure_side_block(ctx, &ctx->minres, &ctx->minres_bytes, minres_layout(ctx, nullptr, &v)));
    minres_layout(ctx, ctx->minres, &v);
    Shard &s = ctx->shards[0];
    hipStream_t st = ctx->stream;
    const int n = ctx->n;
    reset_gemv_stats(ctx);
    const double t_begin = wall_now();

    cgx::MinresArgs a{};
    a.n = n;
    a.nshift = nshift;
    a.lda = ctx->lda;
    a.Y = s.Ap();
    a.k1p = s.k1_part();
    a.nk1p = cgx::plan_partials(s.plan);
    a.X = v.X;
    a.D[0] = v.D[0];
    a.D[1] = v.D[1];
    a.ms = v.ms;
    a.tol = ctx->tol;
    // launch t reads w_t in V[t & 1], v_(t-1) in the other block and the partials wwp[t & 1], and leaves wwp[(t + 1) & 1]
    auto at_launch = [&](int t) {
        a.w = v.V[t & 1];
        a.vprev = v.V[(t + 1) & 1];
        a.ww_in = v.wwp[t & 1];
        a.ww_out = v.wwp[(t + 1) & 1];
        a.t = t;
    };
    at_launch(0);
    a.ww_out = v.wwp[0];
    HIP_TRY(ctx, cgx::launch_minres_init(a, sigma, s.b_full, st));

    // the loop: the step kernel raises the flag when every shift is frozen or the recurrence broke down; it is polled every
    // check_every launches, one batch kept queued, and the launches behind the end write nothing
    const double t0 = wall_now();
    auto launch = [&](int t) -> cgx_status {
        at_launch(t);
        CGX_TRY(run_gemv_plain(ctx, s, a.w));
        HIP_TRY(ctx, cgx::launch_minres_step(a, st));
        return CGX_OK;
    };
    int k = 0;
    CGX_TRY(run_polled(ctx, &v.ms->done, ctx->max_iter, false, launch, &k));
    at_launch(k);
    HIP_TRY(ctx, cgx::launch_minres_close(a, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    const double t_loop = wall_now() - t0;

    // the full width kS, as cgx_solve_shifted: a shift's result must not depend on how many others there are
    CGX_TRY(column_residual_norms(ctx, nshift, kS, v.X, v.Y, v.k1p, v.vm, s.b_full, 0, sigma, v.norms));
    cgx::MinresScalars hm;
    double norms[kS][3];
    HIP_TRY(ctx, hipMemcpyAsync(&hm, v.ms, sizeof hm, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(norms, v.norms, sizeof norms, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    // the last call that can fail: X is written only when the solve succeeds
    HIP_TRY(ctx, hipMemcpy2D(X, (size_t)ldx * sizeof(double), v.X, (size_t)ctx->lda * sizeof(double), (size_t)n * sizeof(double),
                             (size_t)nshift, hipMemcpyDeviceToHost));

    // no K1 statistics: gemv_ms_* and the launch counts stay 0, plain K1 launches are not event-timed
    fill_column_results(ctx, res, nshift, t_begin, t_loop, one_gpu_gemv_bytes(ctx), false, norms, [&](int j) {
        const bool frozen = hm.frozen_at[j] != cgx::kMinresLive;
        // max_iter = 0: no launch ran, so nothing on the device looked at b; b = 0 is solved by x = 0 as it is in launch 0
        const int conv = frozen ? hm.conv[j] : (k == 0 && norms[j][1] == 0.0 ? 1 : 0);
        return ColumnOutcome{frozen ? hm.frozen_at[j] : k, conv, hm.res_prev[j], hm.res_last[j]};
    });
    return CGX_OK;
}

}  // extern "C"
