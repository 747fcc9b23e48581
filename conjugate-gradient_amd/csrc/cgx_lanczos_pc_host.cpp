// cgx_lanczos_pc_host.cpp -- cgx_lanczos_pc, cgx_precond_logdet, cgx_slq_probes and cgx_trace_slq_pc: the preconditioned multi-vector
// Lanczos recurrence (cgx_lanczos_pc.hip) and stochastic Lanczos quadrature on M^-1/2 A M^-1/2.
//
// The recurrence's driver and the estimator are the family's own (lanczos_run, slq_estimate: cgx_lanczos_host.cpp), run with the
// context's preconditioner, or, with none set, on the plain recurrence.  This file holds what only a preconditioner brings: its
// set-up and refusals, log det M, and the probes of covariance M made on the device.  The preconditioner itself -- the inverse
// diagonal, or L, C^-1 and delta -- is the single path's, made by prepare_jacobi / prepare_lowrank once per matrix and shared in
// every direction.  The recurrence's blocks are a side block of their own (cgx_ctx::lanczos_pc), apart from the plain one's.
#include "cgx_internal.h"

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

using namespace cgxi;

namespace {

constexpr int kW = cgx::kMaxRhs;

// the probe maker's kind for the context's preconditioner and the function: log takes covariance M, 1/x covariance I
int probe_kind(const cgx_ctx *ctx, int fn)
{
    if (fn != CGX_SLQ_LOG || ctx->precond == CGX_PRECOND_NONE) return 0;
    return ctx->precond == CGX_PRECOND_JACOBI ? cgx::kLpcJacobi : cgx::kLpcLowrank;
}

// nb library probes (probe0 ...) into dst (column j at + j * lda), on the device
cgx_status make_probes(cgx_ctx *ctx, int kind, unsigned long long seed_mixed, int probe0, int nb, double *dst)
{
    const double *L = nullptr;
    const cgx::LrHead *head = nullptr;
    int rank = 0;
    if (kind == cgx::kLpcLowrank) {
        L = ctx->lr_L;
        rank = ctx->lr_L_rank;
        head = lr_work(ctx).head;
    }
    HIP_TRY(ctx, cgx::launch_lanczos_pc_probes(ctx->n, ctx->lda, nb, kind, seed_mixed, probe0, ctx->shards[0].A, L, rank, head, dst, ctx->stream));
    return CGX_OK;
}

// log det M of the prepared preconditioner.  Jacobi: sum of log A_ii = -log dinv_i in ascending order.  Pivoted Cholesky:
// det(L L^T + delta I) = delta^(n-k) det(delta I + L^T L); the set-up keeps only C^-1, so its host Cholesky, sign flipped.
cgx_status precond_logdet(cgx_ctx *ctx, const std::string &fn, double *out)
{
    hipStream_t st = ctx->stream;
    const int n = ctx->n;
    if (ctx->precond == CGX_PRECOND_JACOBI) {
        std::vector<double> dinv((size_t)n);
        HIP_TRY(ctx, hipMemcpyAsync(dinv.data(), ctx->shards[0].dinv, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
        double s = 0.0;
        for (int i = 0; i < n; ++i) s -= std::log(dinv[i]);
        *out = s;
        return CGX_OK;
    }
    const int k = ctx->lr_L_rank;
    std::vector<double> R((size_t)k * k);
    HIP_TRY(ctx, hipMemcpy2DAsync(R.data(), (size_t)k * sizeof(double), lr_work(ctx).C, (size_t)cgx::kLrLd * sizeof(double),
                                  (size_t)k * sizeof(double), k, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    double logdet_cinv = 0.0;
    for (int c = 0; c < k; ++c) {                          // lower Cholesky in place, column by column
        double d = R[(size_t)c * k + c];
        for (int q = 0; q < c; ++q) d -= R[(size_t)c * k + q] * R[(size_t)c * k + q];
        if (!(d > 0.0) || !std::isfinite(d))
            return fail(ctx, CGX_ERR_BAD_ARG, fn + ": (delta I + L^T L)^-1 of the pivoted-Cholesky factor is not positive definite on the host");
        const double piv = std::sqrt(d);
        R[(size_t)c * k + c] = piv;
        logdet_cinv += 2.0 * std::log(piv);
        for (int r = c + 1; r < k; ++r) {
            double s = R[(size_t)r * k + c];
            for (int q = 0; q < c; ++q) s -= R[(size_t)r * k + q] * R[(size_t)c * k + q];
            R[(size_t)r * k + c] = s / piv;
        }
    }
    *out = (double)(n - k) * std::log(ctx->lr_delta) - logdet_cinv;
    return CGX_OK;
}

}  // namespace

extern "C" {

cgx_status cgx_lanczos_pc(cgx_ctx *ctx, int nvec, int steps, const double *V0, long ldv, double *alpha, double *beta, int *steps_done,
                          double *eta2)
{
    const std::string fn("cgx_lanczos_pc");
    CGX_TRY(check_dense_one_gpu(ctx, fn));
    CGX_TRY(check_lanczos_steps(ctx, fn, steps));
    if (nvec < 1 || nvec > CGX_MAX_RHS) return fail(ctx, CGX_ERR_BAD_ARG, fn + ": nvec must be 1 .. CGX_MAX_RHS");
    if (!V0 || !alpha || !beta || !steps_done || !eta2) return fail(ctx, CGX_ERR_BAD_ARG, fn + ": null pointer");
    if (ldv < ctx->n) return fail(ctx, CGX_ERR_BAD_ARG, fn + ": leading dimension smaller than n");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // M = I: the plain recurrence under cgx_lanczos's name (a bad start vector is reported in its words); eta0^2 = ||V0_j||^2
    if (ctx->precond == CGX_PRECOND_NONE) return lanczos_run(ctx, "cgx_lanczos", false, nvec, steps, V0, ldv, 0, alpha, beta, steps_done, eta2);
    CGX_TRY(prepare_multi_precond(ctx, fn));
    return lanczos_run(ctx, fn, true, nvec, steps, V0, ldv, 0, alpha, beta, steps_done, eta2);
}

cgx_status cgx_precond_logdet(cgx_ctx *ctx, double *logdet)
{
    const std::string fn("cgx_precond_logdet");
    CGX_TRY(check_dense_one_gpu(ctx, fn));
    if (!logdet) return fail(ctx, CGX_ERR_BAD_ARG, fn + ": null pointer");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    *logdet = 0.0;
    if (ctx->precond == CGX_PRECOND_NONE) return CGX_OK;
    CGX_TRY(prepare_multi_precond(ctx, fn));
    return precond_logdet(ctx, fn, logdet);
}

cgx_status cgx_slq_probes(cgx_ctx *ctx, int fn_kind, int nprobe, unsigned long long seed, double *Z, long ldz)
{
    const std::string fn("cgx_slq_probes");
    CGX_TRY(check_dense_one_gpu(ctx, fn));
    if (fn_kind != CGX_SLQ_LOG && fn_kind != CGX_SLQ_INV) return fail(ctx, CGX_ERR_BAD_ARG, fn + ": fn must be CGX_SLQ_LOG or CGX_SLQ_INV");
    if (nprobe < 1 || nprobe > CGX_MAX_PROBES) return fail(ctx, CGX_ERR_BAD_ARG, fn + ": nprobe must be 1 .. CGX_MAX_PROBES");
    if (!Z) return fail(ctx, CGX_ERR_BAD_ARG, fn + ": null pointer");
    if (ldz < ctx->n) return fail(ctx, CGX_ERR_BAD_ARG, fn + ": leading dimension smaller than n");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int kind = probe_kind(ctx, fn_kind);
    if (kind) CGX_TRY(prepare_multi_precond(ctx, fn));
    LanczosView v;
    CGX_TRY(lanczos_block(ctx, true, &v));
    const unsigned long long sm = cgx::hash_mix64(seed);
    for (int j0 = 0; j0 < nprobe; j0 += kW) {
        const int nb = std::min(kW, nprobe - j0);
        CGX_TRY(make_probes(ctx, kind, sm, j0, nb, v.V[0]));
        CGX_TRY(download_columns(ctx, Z + (size_t)j0 * ldz, ldz, v.V[0], nb));
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return CGX_OK;
}

cgx_status cgx_trace_slq_pc(cgx_ctx *ctx, int fn_kind, int nprobe, int steps, unsigned long long seed, const double *Z, long ldz,
                            double *estimate, double *std_error, double *per_probe, double *ritz, double *logdet_precond)
{
    const std::string fn("cgx_trace_slq_pc");
    CGX_TRY(check_dense_one_gpu(ctx, fn));
    CGX_TRY(check_lanczos_steps(ctx, fn, steps));
    CGX_TRY(check_slq_args(ctx, fn, fn_kind, nprobe, estimate, std_error, Z, ldz));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    double logdet_m = 0.0;
    if (ctx->precond == CGX_PRECOND_NONE) {                // M = I: the plain estimator under cgx_trace_slq's name, its host-made probes
        CGX_TRY(slq_estimate(ctx, "cgx_trace_slq", false, fn_kind, nprobe, steps, seed, Z, ldz, nullptr, estimate, std_error, per_probe, ritz));
    } else {
        CGX_TRY(prepare_multi_precond(ctx, fn));
        if (fn_kind == CGX_SLQ_LOG) CGX_TRY(precond_logdet(ctx, fn, &logdet_m));
        LanczosView v;
        CGX_TRY(lanczos_block(ctx, true, &v));
        const int kind = probe_kind(ctx, fn_kind);
        const unsigned long long sm = cgx::hash_mix64(seed);
        const SlqProbes probes = [&](int probe0, int nb) { return make_probes(ctx, kind, sm, probe0, nb, v.V[0]); };
        CGX_TRY(slq_estimate(ctx, fn, true, fn_kind, nprobe, steps, seed, Z, ldz, probes, estimate, std_error, per_probe, ritz));
        *estimate = logdet_m + *estimate;
    }
    if (logdet_precond) *logdet_precond = logdet_m;
    return CGX_OK;
}

}  // extern "C"

