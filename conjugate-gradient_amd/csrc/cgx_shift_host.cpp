// cgx_shift_host.cpp -- cgx_solve_shifted: the host side of multi-shift CG (cgx_shift.hip).
//
// One GPU, dense or CSR storage.  The seed runs in the single path's own buffers with the single path's own loop body
// (enqueue_iteration, cgx_solve.cpp): whatever per-launch K1 the shard's plan names, K3 behind it, and behind K3 the shift kernel.
// Where the context's plan is a persistent kernel nothing of it is touched: the loop below never asks for it, and the next
// cgx_solve_begin sets the state up again from scratch.  The x and p of the shifts, the block of the final verification and the
// shift scalars live in ONE device allocation of the context (cgx_ctx::shift), made on first use and freed with the problem.
#include "cgx_internal.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

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
    int g = 0;
    for (int w = 1; w <= cgx::kMaxRhs; w *= 2) g = std::max(g, cgx::multi_gemv_grid(ctx->n, w));
    size_t off = 0;
    auto take = [&](size_t count) {
        double *p = base ? base + off : nullptr;
        off += (count + 15) / 16 * 16;   // 128-B aligned pieces
        return p;
    };
    v->X = take(vec);
    v->P = take(vec);
    v->Y = take(vec);
    v->k1p = take((size_t)kS * g);
    v->ms = reinterpret_cast<cgx::MultiScalars *>(take((sizeof(cgx::MultiScalars) + 7) / 8));
    v->ss = reinterpret_cast<cgx::ShiftScalars *>(take((sizeof(cgx::ShiftScalars) + 7) / 8));
    return off * sizeof(double);
}

// The context's shift block, made (and zeroed) on first use.
cgx_status ensure_shift(cgx_ctx *ctx, ShiftView *v)
{
    const size_t bytes = shift_layout(ctx, nullptr, v);
    if (!ctx->shift) {
        double *p = nullptr;
        HIP_TRY(ctx, hipMalloc(&p, bytes));
        const cgx_status st = [&]() -> cgx_status {
            HIP_TRY(ctx, hipMemsetAsync(p, 0, bytes, ctx->stream));
            return CGX_OK;
        }();
        if (st != CGX_OK) {
            (void)hipFree(p);
            return st;
        }
        ctx->shift = p;
        ctx->shift_bytes = bytes;
    }
    shift_layout(ctx, ctx->shift, v);
    return CGX_OK;
}

// The checks in the order check_multi (cgx_multi_host.cpp) makes them: context, problem, transport and storage, arguments.
cgx_status check_shifted(cgx_ctx *ctx, int nshift, const double *sigma, const double *X, long ldx)
{
    if (!ctx) return CGX_ERR_BAD_ARG;
    const std::string fn("cgx_solve_shifted");
    if (!ctx->have_matrix) return fail(ctx, CGX_ERR_BAD_ARG, fn + ": no problem set");
    if (ctx->in_solve) return fail(ctx, CGX_ERR_BAD_ARG, fn + ": a cgx_solve_begin / cgx_solve_end pair is open");
    if (ctx->cfg.comm_mode != CGX_COMM_SELF || ctx->nranks != 1 || ctx->shards.size() != 1)
        return fail(ctx, CGX_ERR_UNSUPPORTED, fn + ": one GPU only (CGX_COMM_SELF)");
    if (ctx->banded) return fail(ctx, CGX_ERR_UNSUPPORTED, fn + ": dense or CSR storage only (not CGX_MATRIX_BANDED)");
    if (ctx->precond != CGX_PRECOND_NONE)
        return fail(ctx, CGX_ERR_UNSUPPORTED, fn + ": no preconditioner (it breaks the collinearity of the shifted residuals; "
                                                   "cgx_set_preconditioner)");
    if (ctx->res_forced)
        return fail(ctx, CGX_ERR_UNSUPPORTED, fn + ": the persistent kernels (gemv_variant 40000 / 50000) have no shifted form");
    if (nshift < 1 || nshift > CGX_MAX_SHIFTS) return fail(ctx, CGX_ERR_BAD_ARG, fn + ": nshift must be 1 .. CGX_MAX_SHIFTS");
    if (!sigma || !X) return fail(ctx, CGX_ERR_BAD_ARG, fn + ": null pointer");
    if (ldx < ctx->n) return fail(ctx, CGX_ERR_BAD_ARG, fn + ": leading dimension smaller than n");
    for (int j = 0; j < nshift; ++j)
        if (!(sigma[j] >= 0.0) || !std::isfinite(sigma[j]))
            return fail(ctx, CGX_ERR_BAD_ARG, fn + ": shift " + std::to_string(j) + " is negative or not finite");
    if (!ctx->have_b) return fail(ctx, CGX_ERR_BAD_ARG, fn + ": no source term set");
    return CGX_OK;
}

}  // namespace

extern "C" {

cgx_status cgx_solve_shifted(cgx_ctx *ctx, int nshift, const double *sigma, double *X, long ldx, cgx_result *res)
{
    CGX_TRY(check_shifted(ctx, nshift, sigma, X, ldx));
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
    bool window_open = false;
    if (ctx->cfg.profile_gemv && ctx->max_iter > 0) {
        for (auto &e : ctx->steps_ev)
            if (!e) HIP_TRY(ctx, hipEventCreate(&e));
        HIP_TRY(ctx, hipEventRecord(ctx->steps_ev[0], st));
        window_open = true;
    }
    const int every = std::max(1, ctx->cfg.check_every);
    int k = 0, slot = 0;
    bool pending[2] = {false, false}, stop = false;
    while (k < ctx->max_iter && !stop) {
        const int batch = std::min(ctx->max_iter - k, every);
        for (int i = 0; i < batch; ++i, ++k) {
            CGX_TRY(enqueue_iteration(ctx, k));
            a.k = k;
            HIP_TRY(ctx, cgx::launch_shift_update(a, st));
        }
        HIP_TRY(ctx, hipMemcpyAsync(ctx->h_flags + 2 * slot, &s.sc->done, 2 * sizeof(int), hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipEventRecord(ctx->flag_ev[slot], st));
        pending[slot] = true;
        slot ^= 1;
        if (pending[slot]) {
            HIP_TRY(ctx, hipEventSynchronize(ctx->flag_ev[slot]));
            pending[slot] = false;
            if (ctx->h_flags[2 * slot]) stop = true;
        }
    }
    if (window_open) {
        HIP_TRY(ctx, hipEventRecord(ctx->steps_ev[1], st));
        ctx->steps_ev_pending = true;
    }
    HIP_TRY(ctx, cgx::launch_shift_close(v.ss, a.rrp, a.nrr, nshift, k, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    const double t_loop = wall_now() - t0;

    // the true residuals: Y_j = A x_j (dense: one pass over A for all shifts; CSR: one SpMV per shift), then the norms
    if (ctx->csr) {
        for (int j = 0; j < nshift; ++j)
            HIP_TRY(ctx, cgx::launch_spmv_csr_plain(s.plan, s.csr, s.rows, s.row0, lda, v.X + (size_t)j * lda, v.Y + (size_t)j * lda,
                                                    s.k1_part(), st));
    } else {
        cgx::MultiArgs g{};
        g.A = s.A;
        g.lda = lda;
        g.n = n;
        g.nrhs = kS;   // always the full width: a row's sum order depends on the kernel width, and a shift's result must not
                       // depend on how many others there are (the columns beyond nshift hold zeros or an earlier call's x)
        g.v = v.X;
        g.Y = v.Y;
        g.partials = v.k1p;
        g.ms = v.ms;
        HIP_TRY(ctx, cgx::launch_multi_gemv(g, false, st));
    }
    HIP_TRY(ctx, cgx::launch_shift_norms(n, lda, nshift, v.Y, s.b_full, v.X, v.ss, st));
    cgx::ShiftScalars hs;
    HIP_TRY(ctx, hipMemcpyAsync(&hs, v.ss, sizeof hs, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpy2DAsync(X, (size_t)ldx * sizeof(double), v.X, (size_t)lda * sizeof(double), (size_t)n * sizeof(double), nshift,
                                  hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    if (ctx->ev_used || ctx->upd_used || ctx->steps_ev_pending) CGX_TRY(harvest_gemv_events(ctx));

    if (res) {
        cgx_result base;
        memset(&base, 0, sizeof base);
        base.seconds_solve = wall_now() - t_begin;
        base.seconds_loop = t_loop;
        base.gemv_launches = ctx->gemv_launches;
        base.gemv_ms_avg = ctx->gemv_launches ? ctx->gemv_ms_sum / (double)ctx->gemv_launches : 0.0;
        base.gemv_ms_min = ctx->gemv_ms_min;
        base.gemv_ms_max = ctx->gemv_ms_max;
        base.gemv_discarded = ctx->gemv_discarded;
        base.steps_device_ms = ctx->steps_device_ms;
        if (!ctx->gemv_samples.empty()) {
            std::vector<float> sm(ctx->gemv_samples);
            const size_t mid = sm.size() / 2;
            std::nth_element(sm.begin(), sm.begin() + mid, sm.end());
            double med = sm[mid];
            if (sm.size() % 2 == 0) med = 0.5 * (med + *std::max_element(sm.begin(), sm.begin() + mid));
            base.gemv_ms_median = med;
        }
        base.gemv_bytes = ctx->csr ? 12.0 * (double)s.csr.nnz + 8.0 * ((double)s.rows + 1) + 8.0 * s.rows + 8.0 * n
                                   : 8.0 * ((double)s.rows * n + n + s.rows);
        for (int j = 0; j < nshift; ++j) {
            cgx_result &o = res[j];
            o = base;
            const bool frozen = hs.frozen_at[j] != cgx::kShiftLive;
            o.iterations = frozen ? hs.frozen_at[j] : k;
            o.converged = frozen ? 1 : 0;
            o.residual_prev = hs.res_prev[j];
            o.residual_last = hs.res_last[j];
            o.x_norm = std::sqrt(hs.norms[j][2]);
            o.rel_residual = std::sqrt(hs.norms[j][0]) / std::sqrt(hs.norms[j][1]);
        }
    }
    return CGX_OK;
}

}  // extern "C"
