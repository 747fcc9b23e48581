// cgx_lanczos_host.cpp -- cgx_lanczos and cgx_trace_slq, and the two pieces every host of the Lanczos family runs on: THE driver of
// the multi-vector recurrence (lanczos_run: cgx_lanczos.hip, or with the context's preconditioner cgx_lanczos_pc.hip) and THE
// stochastic Lanczos quadrature on top of it (slq_estimate).  DESIGN.md sections 17 and 18; the Jacobi-matrix arithmetic is
// cgx_tridiag.cpp.
//
// One GPU, dense storage.  The blocks of a recurrence live in ONE device allocation of the context (cgx_ctx::lanczos; preconditioned
// cgx_ctx::lanczos_pc), apart from the single path's buffers and from the multi blocks, made on the first call of a problem and freed
// with it.  A step is the plain multi-vector K1 of cgx_multi.hip as it is, then the recurrence's step kernel(s), and nothing is
// polled: the steps are queued behind each other and one synchronisation ends them.
#include "cgx_internal.h"

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

using namespace cgxi;

namespace {

constexpr int kW = cgx::kMaxRhs;
constexpr int kSlqBatch = 8;   // probes per Lanczos run: the width at which K1m is cheapest per column

size_t lanczos_layout(const cgx_ctx *ctx, bool pc, double *base, LanczosView *v)
{
    const size_t vec = (size_t)kW * ctx->lda, g3 = (size_t)cgx::multi_update_grid(ctx->n);
    Carver c{base};
    v->V[0] = c.take(vec);
    v->V[1] = c.take(vec);
    v->U = pc ? c.take(vec) : nullptr;
    v->Y = c.take(vec);
    v->k1p = c.take((size_t)kW * k1p_stride(ctx->n));
    v->wwp[0] = c.take((size_t)kW * g3);
    v->wwp[1] = c.take((size_t)kW * g3);
    v->tpart = pc ? c.take((size_t)kW * g3 * cgx::kLrLd) : nullptr;
    v->alpha = c.take((size_t)kW * cgx::kMaxLanczosSteps);
    v->beta = c.take((size_t)kW * cgx::kMaxLanczosSteps);
    v->ls = c.take_struct<cgx::LanczosScalars>();
    return c.bytes();
}

// What stays over the steps of a run.  The preconditioned kernels' block serves both recurrences: the plain one's is its head.
cgx::LanczosPcArgs run_args(const cgx_ctx *ctx, const LanczosView &v, bool pc, int nvec)
{
    cgx::LanczosPcArgs a{};
    a.n = ctx->n;
    a.nvec = nvec;
    a.lda = ctx->lda;
    a.u = v.U;
    a.Y = v.Y;
    a.k1p = v.k1p;
    a.g1 = cgx::multi_gemv_grid(ctx->n, cgx::multi_width(nvec));
    a.ls = v.ls;
    a.alpha = v.alpha;
    a.beta = v.beta;
    if (pc) a.M = pc_factor(ctx, v.tpart);
    return a;
}

cgx::LanczosArgs plain_step(const cgx::LanczosPcArgs &a)
{
    return cgx::LanczosArgs{a.n, a.nvec, a.lda, a.w, a.vprev, a.Y, a.k1p, a.g1, a.wu_in, a.wu_out, a.ls, a.alpha, a.beta, a.t};
}

}  // namespace

cgx_status cgxi::check_lanczos_steps(cgx_ctx *ctx, const std::string &fn, int steps)
{
    if (steps < 1 || steps > CGX_MAX_LANCZOS_STEPS || steps > ctx->n)
        return fail(ctx, CGX_ERR_BAD_ARG, fn + ": steps must be 1 .. min(n, CGX_MAX_LANCZOS_STEPS)");
    return CGX_OK;
}

cgx_status cgxi::check_lanczos(cgx_ctx *ctx, const std::string &fn, int steps)
{
    CGX_TRY(check_dense_one_gpu(ctx, fn));
    if (ctx->precond != CGX_PRECOND_NONE)
        return fail(ctx, CGX_ERR_UNSUPPORTED, fn + ": a preconditioner is set and would be ignored (cgx_set_preconditioner)");
    return check_lanczos_steps(ctx, fn, steps);
}

cgx_status cgxi::lanczos_block(cgx_ctx *ctx, bool pc, LanczosView *v)
{
    double **block = pc ? &ctx->lanczos_pc : &ctx->lanczos;
    CGX_TRY(ensure_side_block(ctx, block, pc ? &ctx->lanczos_pc_bytes : &ctx->lanczos_bytes, lanczos_layout(ctx, pc, nullptr, v)));
    lanczos_layout(ctx, pc, *block, v);
    return CGX_OK;
}

cgx_status cgxi::lanczos_run(cgx_ctx *ctx, const std::string &fn, bool pc, int nvec, int steps, const double *V0, long ldv, int col0,
                             double *alpha, double *beta, int *m, double *z2, double *basis)
{
    LanczosView v;
    CGX_TRY(lanczos_block(ctx, pc, &v));
    hipStream_t st = ctx->stream;
    const int n = ctx->n;
    const long lda = ctx->lda;
    cgx::LanczosPcArgs a = run_args(ctx, v, pc, nvec);

    if (V0) CGX_TRY(upload_columns(ctx, v.V[0], V0, ldv, nvec));
    a.w = v.V[0];
    a.vprev = v.V[1];
    a.wu_in = v.wwp[1];
    a.wu_out = v.wwp[0];
    if (pc) HIP_TRY(ctx, cgx::launch_lanczos_pc_init(a, st));
    else HIP_TRY(ctx, cgx::launch_lanczos_init(n, lda, nvec, a.w, a.vprev, a.wu_out, v.ls, st));
    for (int t = 0; t < steps; ++t) {
        a.w = v.V[t & 1];
        a.vprev = v.V[(t + 1) & 1];
        a.wu_in = v.wwp[t & 1];
        a.wu_out = v.wwp[(t + 1) & 1];
        a.t = t;
        HIP_TRY(ctx, cgx::launch_multi_gemv(plain_k1m_args(ctx, nvec, pc ? v.U : a.w, v.Y, v.k1p), false, st));
        if (pc) HIP_TRY(ctx, cgx::launch_lanczos_pc_step(a, st));
        else HIP_TRY(ctx, cgx::launch_lanczos_step(plain_step(a), st));
        if (basis)
            HIP_TRY(ctx, hipMemcpyAsync(basis + (size_t)t * nvec * lda, a.w, (size_t)nvec * lda * sizeof(double), hipMemcpyDeviceToDevice, st));
    }
    if (pc) HIP_TRY(ctx, cgx::launch_lanczos_pc_close(n, nvec, steps, v.wwp[steps & 1], v.ls, v.beta, st));
    else HIP_TRY(ctx, cgx::launch_lanczos_close(n, nvec, steps, v.wwp[steps & 1], v.ls, v.beta, st));
    cgx::LanczosScalars hs;
    HIP_TRY(ctx, hipMemcpyAsync(&hs, v.ls, sizeof hs, hipMemcpyDeviceToHost, st));
    const size_t row = (size_t)steps * sizeof(double), pitch = (size_t)cgx::kMaxLanczosSteps * sizeof(double);
    HIP_TRY(ctx, hipMemcpy2DAsync(alpha, row, v.alpha, pitch, row, nvec, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpy2DAsync(beta, row, v.beta, pitch, row, nvec, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));

    for (int j = 0; j < nvec; ++j)
        if (hs.bad[j])
            return fail(ctx, CGX_ERR_BAD_ARG, fn + ": start vector " + std::to_string(col0 + j) +
                                                  (pc ? " has M^-1 norm 0 or is not finite" : " has norm 0 or is not finite"));
    for (int j = 0; j < nvec; ++j) {
        m[j] = hs.m[j];
        z2[j] = hs.z2[j];
        for (int t = m[j]; t < steps; ++t) alpha[(size_t)j * steps + t] = beta[(size_t)j * steps + t] = 0.0;
    }
    return CGX_OK;
}

cgx_status cgxi::check_slq_args(cgx_ctx *ctx, const std::string &fn, int fn_kind, int nprobe, const double *estimate,
                                const double *std_error, const double *Z, long ldz)
{
    if (fn_kind != CGX_SLQ_LOG && fn_kind != CGX_SLQ_INV) return fail(ctx, CGX_ERR_BAD_ARG, fn + ": fn must be CGX_SLQ_LOG or CGX_SLQ_INV");
    if (nprobe < 1 || nprobe > CGX_MAX_PROBES) return fail(ctx, CGX_ERR_BAD_ARG, fn + ": nprobe must be 1 .. CGX_MAX_PROBES");
    if (!estimate || !std_error) return fail(ctx, CGX_ERR_BAD_ARG, fn + ": null pointer");
    if (Z && ldz < ctx->n) return fail(ctx, CGX_ERR_BAD_ARG, fn + ": leading dimension smaller than n");
    return CGX_OK;
}

cgx_status cgxi::slq_estimate(cgx_ctx *ctx, const std::string &fn, bool pc, int fn_kind, int nprobe, int steps, unsigned long long seed,
                              const double *Z, long ldz, const SlqProbes &device_probes, double *estimate, double *std_error,
                              double *per_probe, double *ritz)
{
    const int n = ctx->n;
    const unsigned long long sm = cgx::hash_mix64(seed);
    std::vector<double> block, value((size_t)nprobe), alpha((size_t)kSlqBatch * steps), beta((size_t)kSlqBatch * steps);
    std::vector<double> theta((size_t)steps), weight((size_t)steps);
    if (!Z && !device_probes) block.resize((size_t)kSlqBatch * n);
    double lo = HUGE_VAL, hi = -HUGE_VAL;
    for (int j0 = 0; j0 < nprobe; j0 += kSlqBatch) {
        const int nb = std::min(kSlqBatch, nprobe - j0);
        const double *V0 = Z ? Z + (size_t)j0 * ldz : nullptr;   // null: the probes are on the device already
        if (!Z && device_probes) CGX_TRY(device_probes(j0, nb));
        if (!Z && !device_probes) {
            for (int j = 0; j < nb; ++j)
                for (int i = 0; i < n; ++i)
                    block[(size_t)j * n + i] = cgx::rademacher_sign(sm, (unsigned long long)(j0 + j), (unsigned long long)i);
            V0 = block.data();
        }
        int m[kSlqBatch];
        double z2[kSlqBatch];
        CGX_TRY(lanczos_run(ctx, fn, pc, nb, steps, V0, Z ? ldz : (long)n, j0, alpha.data(), beta.data(), m, z2));
        for (int j = 0; j < nb; ++j) {
            const double *a = alpha.data() + (size_t)j * steps, *b = beta.data() + (size_t)j * steps;
            if (m[j] < 1 || !finite_entries(m[j], a, b) || !gauss_rule(m[j], a, b, theta.data(), weight.data()))
                return fail(ctx, CGX_ERR_BAD_ARG, fn + ": the Lanczos coefficients of probe " + std::to_string(j0 + j) +
                                                      " are not finite, or their Jacobi matrix has no eigen-decomposition");
            if (!(theta[0] > 0.0))
                return fail(ctx, CGX_ERR_BAD_ARG, fn + ": matrix is not positive definite (Ritz value " + std::to_string(theta[0]) +
                                                      " from probe " + std::to_string(j0 + j) + ")");
            double q = 0.0;
            for (int i = 0; i < m[j]; ++i) q += weight[i] * (fn_kind == CGX_SLQ_LOG ? std::log(theta[i]) : 1.0 / theta[i]);   // ascending theta
            value[(size_t)j0 + j] = z2[j] * q;
            lo = std::min(lo, theta[0]);
            hi = std::max(hi, theta[m[j] - 1]);
        }
    }
    double mean = 0.0;
    for (int j = 0; j < nprobe; ++j) mean += value[j];
    mean /= nprobe;
    double var = 0.0;
    for (int j = 0; j < nprobe; ++j) var += (value[j] - mean) * (value[j] - mean);
    *estimate = mean;
    *std_error = nprobe > 1 ? std::sqrt(var / (nprobe - 1)) / std::sqrt((double)nprobe) : 0.0;
    if (per_probe) memcpy(per_probe, value.data(), (size_t)nprobe * sizeof(double));
    if (ritz) { ritz[0] = lo; ritz[1] = hi; }
    return CGX_OK;
}

extern "C" {

cgx_status cgx_lanczos(cgx_ctx *ctx, int nvec, int steps, const double *V0, long ldv, double *alpha, double *beta, int *steps_done)
{
    const std::string fn("cgx_lanczos");
    CGX_TRY(check_lanczos(ctx, fn, steps));
    if (nvec < 1 || nvec > CGX_MAX_RHS) return fail(ctx, CGX_ERR_BAD_ARG, fn + ": nvec must be 1 .. CGX_MAX_RHS");
    if (!V0 || !alpha || !beta || !steps_done) return fail(ctx, CGX_ERR_BAD_ARG, fn + ": null pointer");
    if (ldv < ctx->n) return fail(ctx, CGX_ERR_BAD_ARG, fn + ": leading dimension smaller than n");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    double z2[kW];
    return lanczos_run(ctx, fn, false, nvec, steps, V0, ldv, 0, alpha, beta, steps_done, z2);
}

cgx_status cgx_trace_slq(cgx_ctx *ctx, int fn, int nprobe, int steps, unsigned long long seed, const double *Z, long ldz,
                         double *estimate, double *std_error, double *per_probe, double *ritz)
{
    const std::string name("cgx_trace_slq");
    CGX_TRY(check_lanczos(ctx, name, steps));
    CGX_TRY(check_slq_args(ctx, name, fn, nprobe, estimate, std_error, Z, ldz));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return slq_estimate(ctx, name, false, fn, nprobe, steps, seed, Z, ldz, nullptr, estimate, std_error, per_probe, ritz);
}

}  // extern "C"
