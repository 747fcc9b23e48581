// cgx_lanczos_pc_host.cpp -- cgx_lanczos_pc, cgx_precond_logdet, cgx_slq_probes and cgx_trace_slq_pc: the host side of the
// preconditioned multi-vector Lanczos recurrence (cgx_lanczos_pc.hip) and of stochastic Lanczos quadrature on M^-1/2 A M^-1/2
// (DESIGN.md section 18).
//
// One GPU, dense storage.  The blocks live in ONE device allocation of the context (cgx_ctx::lanczos_pc), apart from the single
// path's buffers, the multi blocks and the plain recurrence's block.  The preconditioner itself -- the inverse diagonal, or L, C^-1
// and delta -- is the single path's, made by prepare_jacobi / prepare_lowrank once per matrix and shared in every direction.  A
// step is the plain multi-vector K1 of cgx_multi.hip as it is, then one (Jacobi) or two (pivoted Cholesky) launches of
// cgx_lanczos_pc.hip; nothing is polled: the steps are queued behind each other and one synchronisation ends them.
#include "cgx_internal.h"

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

using namespace cgxi;

namespace {

constexpr int kW = cgx::kMaxRhs;
constexpr int kSlqBatch = 8;   // probes per Lanczos run, as cgx_trace_slq

struct LpcView {
    double *V[2], *U, *Y;           // kW x lda each (column j at + j * lda): w / v_prev in ping-pong, u = M^-1 w, A u
    double *k1p;                    // kW x k1p_stride(n): K1m's u.Au partials
    double *wup[2];                 // kW x multi_update_grid(n) each: the w.u partials, ping-pong over the steps
    double *tpart;                  // kW x lr_grid(n) x kLrLd: the partials of L^T w (pivoted Cholesky)
    double *alpha, *beta;           // kW x kMaxLanczosSteps each: the histories
    cgx::LanczosScalars *ls;
};

size_t lpc_layout(const cgx_ctx *ctx, double *base, LpcView *v)
{
    const size_t vec = (size_t)kW * ctx->lda, g3 = (size_t)cgx::multi_update_grid(ctx->n);
    Carver c{base};
    v->V[0] = c.take(vec);
    v->V[1] = c.take(vec);
    v->U = c.take(vec);
    v->Y = c.take(vec);
    v->k1p = c.take((size_t)kW * k1p_stride(ctx->n));
    v->wup[0] = c.take((size_t)kW * g3);
    v->wup[1] = c.take((size_t)kW * g3);
    v->tpart = c.take((size_t)kW * g3 * cgx::kLrLd);
    v->alpha = c.take((size_t)kW * cgx::kMaxLanczosSteps);
    v->beta = c.take((size_t)kW * cgx::kMaxLanczosSteps);
    v->ls = c.take_struct<cgx::LanczosScalars>();
    return c.bytes();
}

cgx_status ensure_lpc(cgx_ctx *ctx, LpcView *v)
{
    CGX_TRY(ensure_side_block(ctx, &ctx->lanczos_pc, &ctx->lanczos_pc_bytes, lpc_layout(ctx, nullptr, v)));
    lpc_layout(ctx, ctx->lanczos_pc, v);
    return CGX_OK;
}

// The checks every entry point here begins with, in cgx_solve_multi_pc's order: context, problem, transport, storage.
cgx_status check_scope(cgx_ctx *ctx, const std::string &fn)
{
    CGX_TRY(check_one_gpu_call(ctx, fn));
    if (ctx->sparse()) return fail(ctx, CGX_ERR_UNSUPPORTED, fn + ": dense storage only (CGX_MATRIX_DENSE)");
    return CGX_OK;
}

cgx_status check_steps(cgx_ctx *ctx, const std::string &fn, int steps)
{
    if (steps < 1 || steps > CGX_MAX_LANCZOS_STEPS || steps > ctx->n)
        return fail(ctx, CGX_ERR_BAD_ARG, fn + ": steps must be 1 .. min(n, CGX_MAX_LANCZOS_STEPS)");
    return CGX_OK;
}

// The preconditioner, behind the argument checks: cgx_solve_multi_pc's refusals with their status and message, and -- once per
// matrix (rank, shift) -- the inverse diagonal or the factor, by the single path's own functions.
cgx_status prepare_pc(cgx_ctx *ctx, const std::string &fn)
{
    if (ctx->precond == CGX_PRECOND_JACOBI) {
        if (ctx->precond_block > 1)
            return fail(ctx, CGX_ERR_UNSUPPORTED, fn + ": block Jacobi (cgx_set_preconditioner_block > 1) has no multi-vector update kernel; "
                                                       "point Jacobi and CGX_PRECOND_PIVCHOL have");
        return prepare_jacobi(ctx);
    }
    if (ctx->precond == CGX_PRECOND_PIVCHOL) return prepare_lowrank(ctx);
    return fail(ctx, CGX_ERR_UNSUPPORTED, fn + ": unknown preconditioner");
}

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

// THE recurrence: nvec start vectors through `steps` steps.  V0 (one per row, pitch ldv) is uploaded, or, V0 == nullptr, the block
// v.V[0] is taken as the caller left it on the device.  alpha, beta: nvec rows of `steps` doubles, zero at t >= m[j]; eta2[j] =
// w_0 . M^-1 w_0 as the device summed it.  col0: the number of row 0 in the caller's own count, for the message about a bad vector.
cgx_status lpc_run(cgx_ctx *ctx, const std::string &fn, const LpcView &v, int nvec, int steps, const double *V0, long ldv, int col0,
                   double *alpha, double *beta, int *m, double *eta2)
{
    hipStream_t st = ctx->stream;
    const int n = ctx->n;
    const long lda = ctx->lda;
    cgx::LanczosPcArgs a{};
    a.n = n;
    a.nvec = nvec;
    a.lda = lda;
    a.u = v.U;
    a.Y = v.Y;
    a.k1p = v.k1p;
    a.g1 = cgx::multi_gemv_grid(n, cgx::multi_width(nvec));
    a.ls = v.ls;
    a.alpha = v.alpha;
    a.beta = v.beta;
    if (ctx->precond == CGX_PRECOND_JACOBI) {
        a.dinv = ctx->shards[0].dinv;
    } else {
        const cgx::LrWork w = lr_work(ctx);
        a.L = ctx->lr_L;
        a.rank = ctx->lr_L_rank;
        a.Cinv = w.C;
        a.head = w.head;
        a.tpart = v.tpart;
    }
    if (V0)
        HIP_TRY(ctx, hipMemcpy2DAsync(v.V[0], (size_t)lda * sizeof(double), V0, (size_t)ldv * sizeof(double), (size_t)n * sizeof(double), nvec,
                                      hipMemcpyHostToDevice, st));
    a.w = v.V[0];
    a.vprev = v.V[1];
    a.wu_in = v.wup[1];
    a.wu_out = v.wup[0];
    HIP_TRY(ctx, cgx::launch_lanczos_pc_init(a, st));
    for (int t = 0; t < steps; ++t) {
        cgx::MultiArgs g{};
        g.A = ctx->shards[0].A;
        g.lda = lda;
        g.n = n;
        g.nrhs = nvec;
        g.v = v.U;
        g.Y = v.Y;
        g.partials = v.k1p;
        HIP_TRY(ctx, cgx::launch_multi_gemv(g, false, st));
        a.w = v.V[t & 1];
        a.vprev = v.V[(t + 1) & 1];
        a.wu_in = v.wup[t & 1];
        a.wu_out = v.wup[(t + 1) & 1];
        a.t = t;
        HIP_TRY(ctx, cgx::launch_lanczos_pc_step(a, st));
    }
    HIP_TRY(ctx, cgx::launch_lanczos_pc_close(n, nvec, steps, v.wup[steps & 1], v.ls, v.beta, st));
    cgx::LanczosScalars hs;
    HIP_TRY(ctx, hipMemcpyAsync(&hs, v.ls, sizeof hs, hipMemcpyDeviceToHost, st));
    const size_t row = (size_t)steps * sizeof(double), pitch = (size_t)cgx::kMaxLanczosSteps * sizeof(double);
    HIP_TRY(ctx, hipMemcpy2DAsync(alpha, row, v.alpha, pitch, row, nvec, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpy2DAsync(beta, row, v.beta, pitch, row, nvec, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));

    for (int j = 0; j < nvec; ++j)
        if (hs.bad[j])
            return fail(ctx, CGX_ERR_BAD_ARG, fn + ": start vector " + std::to_string(col0 + j) + " has M^-1 norm 0 or is not finite");
    for (int j = 0; j < nvec; ++j) {
        m[j] = hs.m[j];
        eta2[j] = hs.z2[j];
        for (int t = m[j]; t < steps; ++t) alpha[(size_t)j * steps + t] = beta[(size_t)j * steps + t] = 0.0;
    }
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
    CGX_TRY(check_scope(ctx, fn));
    CGX_TRY(check_steps(ctx, fn, steps));
    if (nvec < 1 || nvec > CGX_MAX_RHS) return fail(ctx, CGX_ERR_BAD_ARG, fn + ": nvec must be 1 .. CGX_MAX_RHS");
    if (!V0 || !alpha || !beta || !steps_done || !eta2) return fail(ctx, CGX_ERR_BAD_ARG, fn + ": null pointer");
    if (ldv < ctx->n) return fail(ctx, CGX_ERR_BAD_ARG, fn + ": leading dimension smaller than n");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (ctx->precond == CGX_PRECOND_NONE) {                // cgx_lanczos itself; eta0^2 = ||V0_j||^2 as its device code sums it
        CGX_TRY(cgx_lanczos(ctx, nvec, steps, V0, ldv, alpha, beta, steps_done));
        // (the plain recurrence's scalars are the last piece of its block, and their size is a whole number of the Carver's pieces)
        static_assert(sizeof(cgx::LanczosScalars) % 128 == 0, "LanczosScalars must end its side block exactly");
        cgx::LanczosScalars hs;
        HIP_TRY(ctx, hipMemcpy(&hs, reinterpret_cast<const char *>(ctx->lanczos) + ctx->lanczos_bytes - sizeof hs, sizeof hs, hipMemcpyDeviceToHost));
        for (int j = 0; j < nvec; ++j) eta2[j] = hs.z2[j];
        return CGX_OK;
    }
    CGX_TRY(prepare_pc(ctx, fn));
    LpcView v;
    CGX_TRY(ensure_lpc(ctx, &v));
    return lpc_run(ctx, fn, v, nvec, steps, V0, ldv, 0, alpha, beta, steps_done, eta2);
}

cgx_status cgx_precond_logdet(cgx_ctx *ctx, double *logdet)
{
    const std::string fn("cgx_precond_logdet");
    CGX_TRY(check_scope(ctx, fn));
    if (!logdet) return fail(ctx, CGX_ERR_BAD_ARG, fn + ": null pointer");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    *logdet = 0.0;
    if (ctx->precond == CGX_PRECOND_NONE) return CGX_OK;
    CGX_TRY(prepare_pc(ctx, fn));
    return precond_logdet(ctx, fn, logdet);
}

cgx_status cgx_slq_probes(cgx_ctx *ctx, int fn_kind, int nprobe, unsigned long long seed, double *Z, long ldz)
{
    const std::string fn("cgx_slq_probes");
    CGX_TRY(check_scope(ctx, fn));
    if (fn_kind != CGX_SLQ_LOG && fn_kind != CGX_SLQ_INV) return fail(ctx, CGX_ERR_BAD_ARG, fn + ": fn must be CGX_SLQ_LOG or CGX_SLQ_INV");
    if (nprobe < 1 || nprobe > CGX_MAX_PROBES) return fail(ctx, CGX_ERR_BAD_ARG, fn + ": nprobe must be 1 .. CGX_MAX_PROBES");
    if (!Z) return fail(ctx, CGX_ERR_BAD_ARG, fn + ": null pointer");
    if (ldz < ctx->n) return fail(ctx, CGX_ERR_BAD_ARG, fn + ": leading dimension smaller than n");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int kind = probe_kind(ctx, fn_kind);
    if (kind) CGX_TRY(prepare_pc(ctx, fn));
    LpcView v;
    CGX_TRY(ensure_lpc(ctx, &v));
    const unsigned long long sm = cgx::hash_mix64(seed);
    for (int j0 = 0; j0 < nprobe; j0 += kW) {
        const int nb = std::min(kW, nprobe - j0);
        CGX_TRY(make_probes(ctx, kind, sm, j0, nb, v.V[0]));
        HIP_TRY(ctx, hipMemcpy2DAsync(Z + (size_t)j0 * ldz, (size_t)ldz * sizeof(double), v.V[0], (size_t)ctx->lda * sizeof(double),
                                      (size_t)ctx->n * sizeof(double), nb, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return CGX_OK;
}

cgx_status cgx_trace_slq_pc(cgx_ctx *ctx, int fn_kind, int nprobe, int steps, unsigned long long seed, const double *Z, long ldz,
                            double *estimate, double *std_error, double *per_probe, double *ritz, double *logdet_precond)
{
    const std::string fn("cgx_trace_slq_pc");
    CGX_TRY(check_scope(ctx, fn));
    CGX_TRY(check_steps(ctx, fn, steps));
    if (fn_kind != CGX_SLQ_LOG && fn_kind != CGX_SLQ_INV) return fail(ctx, CGX_ERR_BAD_ARG, fn + ": fn must be CGX_SLQ_LOG or CGX_SLQ_INV");
    if (nprobe < 1 || nprobe > CGX_MAX_PROBES) return fail(ctx, CGX_ERR_BAD_ARG, fn + ": nprobe must be 1 .. CGX_MAX_PROBES");
    if (!estimate || !std_error) return fail(ctx, CGX_ERR_BAD_ARG, fn + ": null pointer");
    if (Z && ldz < ctx->n) return fail(ctx, CGX_ERR_BAD_ARG, fn + ": leading dimension smaller than n");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (ctx->precond == CGX_PRECOND_NONE) {                // cgx_trace_slq itself, M = I
        CGX_TRY(cgx_trace_slq(ctx, fn_kind, nprobe, steps, seed, Z, ldz, estimate, std_error, per_probe, ritz));
        if (logdet_precond) *logdet_precond = 0.0;
        return CGX_OK;
    }
    CGX_TRY(prepare_pc(ctx, fn));
    double logdet_m = 0.0;
    if (fn_kind == CGX_SLQ_LOG) CGX_TRY(precond_logdet(ctx, fn, &logdet_m));
    LpcView v;
    CGX_TRY(ensure_lpc(ctx, &v));

    const int kind = probe_kind(ctx, fn_kind);
    const unsigned long long sm = cgx::hash_mix64(seed);
    std::vector<double> value((size_t)nprobe), alpha((size_t)kSlqBatch * steps), beta((size_t)kSlqBatch * steps);
    std::vector<double> theta((size_t)steps), weight((size_t)steps);
    double lo = HUGE_VAL, hi = -HUGE_VAL;
    for (int j0 = 0; j0 < nprobe; j0 += kSlqBatch) {
        const int nb = std::min(kSlqBatch, nprobe - j0);
        if (!Z) CGX_TRY(make_probes(ctx, kind, sm, j0, nb, v.V[0]));
        int m[kSlqBatch];
        double eta2[kSlqBatch];
        CGX_TRY(lpc_run(ctx, fn, v, nb, steps, Z ? Z + (size_t)j0 * ldz : nullptr, ldz, j0, alpha.data(), beta.data(), m, eta2));
        for (int j = 0; j < nb; ++j) {
            const double *a = alpha.data() + (size_t)j * steps, *b = beta.data() + (size_t)j * steps;
            if (m[j] < 1 || cgx_tridiag_quadrature(m[j], a, b, theta.data(), weight.data()) != CGX_OK)
                return fail(ctx, CGX_ERR_BAD_ARG, fn + ": the Lanczos coefficients of probe " + std::to_string(j0 + j) +
                                                      " are not finite, or their Jacobi matrix has no eigen-decomposition");
            if (!(theta[0] > 0.0))
                return fail(ctx, CGX_ERR_BAD_ARG, fn + ": matrix is not positive definite (Ritz value " + std::to_string(theta[0]) +
                                                      " from probe " + std::to_string(j0 + j) + ")");
            double q = 0.0;
            for (int i = 0; i < m[j]; ++i) q += weight[i] * (fn_kind == CGX_SLQ_LOG ? std::log(theta[i]) : 1.0 / theta[i]);   // ascending theta
            value[(size_t)j0 + j] = eta2[j] * q;
            lo = std::min(lo, theta[0]);
            hi = std::max(hi, theta[m[j] - 1]);
        }
    }
    double mean = 0.0;
    for (int j = 0; j < nprobe; ++j) mean += value[j];
    mean /= nprobe;
    double var = 0.0;
    for (int j = 0; j < nprobe; ++j) var += (value[j] - mean) * (value[j] - mean);
    *estimate = logdet_m + mean;
    *std_error = nprobe > 1 ? std::sqrt(var / (nprobe - 1)) / std::sqrt((double)nprobe) : 0.0;
    if (per_probe) memcpy(per_probe, value.data(), (size_t)nprobe * sizeof(double));
    if (ritz) { ritz[0] = lo; ritz[1] = hi; }
    if (logdet_precond) *logdet_precond = logdet_m;
    return CGX_OK;
}

}  // extern "C"
