// cgx_funm_host.cpp -- cgx_apply_function and cgx_probe_funm_combine: f(A) b by Lanczos.
//
// One GPU, dense storage, no preconditioner.  The recurrence is cgx_lanczos's own (lanczos_run, cgx_lanczos_host.cpp) with one
// device-to-device copy behind every step that keeps the normalised v_t; one synchronisation ends it.  The coefficients
// ||b_j|| f(T_j) e_1 and the lagged ones behind change[] are made on the host (tridiag_function, cgx_tridiag.cpp: O(m^2) per
// column), go up with the step counts, and one launch of k_funm_combine (cgx_funm.hip) sums the basis.  The table, the step counts,
// the result block and the basis live in ONE device allocation of the context (cgx_ctx::funm), apart from every other path's buffers.
#include "cgx_internal.h"

#include <cmath>
#include <string>
#include <system_error>
#include <thread>
#include <vector>

using namespace cgxi;

namespace {

constexpr int kW = cgx::kMaxRhs;
constexpr int kThreadedSteps = 64;   // below it a call's coefficient work is shorter than starting the threads

struct FunmView {
    double *C;                      // kW x kMaxLanczosSteps: the coefficient table (row j at + j * steps of the call)
    int *m;                         // kW step counts
    double *X;                      // kW x lda: the result block (column j at + j * lda)
    double *Q;                      // steps x nvec x lda of the call: the basis, last so that the fixed pieces stay where they are
};

size_t funm_layout(const cgx_ctx *ctx, double *base, int nvec, int steps, FunmView *v)
{
    Carver c{base};
    v->C = c.take((size_t)kW * cgx::kMaxLanczosSteps);
    v->m = reinterpret_cast<int *>(c.take(kW));
    v->X = c.take((size_t)kW * ctx->lda);
    v->Q = c.take((size_t)steps * nvec * ctx->lda);
    return c.bytes();
}

// The block for a call of (nvec, steps): made on first use, made again when this call needs more than it holds.
cgx_status ensure_funm(cgx_ctx *ctx, const std::string &fn, int nvec, int steps, FunmView *v)
{
    CGX_TRY(ensure_growing_block(ctx, &ctx->funm, &ctx->funm_bytes, funm_layout(ctx, nullptr, nvec, steps, v), fn,
                                 "8 steps nvec lda = " + std::to_string(steps) + " x " + std::to_string(nvec) + " x " +
                                     std::to_string(ctx->lda) + " doubles"));
    funm_layout(ctx, ctx->funm, nvec, steps, v);
    return CGX_OK;
}

cgx_status run_combine(cgx_ctx *ctx, const FunmView &v, int nvec, int steps, const double *coef, const int *m, double *X, long ldx)
{
    hipStream_t st = ctx->stream;
    HIP_TRY(ctx, hipMemcpyAsync(v.C, coef, (size_t)nvec * steps * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(v.m, m, (size_t)nvec * sizeof(int), hipMemcpyHostToDevice, st));
    cgx::FunmArgs a{};
    a.n = ctx->n;
    a.nvec = nvec;
    a.steps = steps;
    a.lda = ctx->lda;
    a.Q = v.Q;
    a.C = v.C;
    a.m = v.m;
    a.X = v.X;
    a.ldx = ctx->lda;
    HIP_TRY(ctx, cgx::launch_funm_combine(a, st));
    CGX_TRY(download_columns(ctx, X, ldx, v.X, nvec));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return CGX_OK;
}

// One column behind the recurrence: c = sqrt(z2) f(T_m) e_1 into cj (m entries; the caller zeroed the rest), and the indicator
// change = || c(m) - pad(c(lag)) || / || c(m) || with c(lag) from the leading lag x lag block, lag = m - max(1, m / 8); sums in
// ascending t, each product rounded by itself.
struct ColumnCoef {
    TridiagFn status = TridiagFn::ok;
    double bad = 0.0;                // the Ritz value outside the function's domain
    double change = 1.0;
};

ColumnCoef column_coefficients(int m, const double *a, const double *b, int fn, double param, double z2, double *cj)
{
    ColumnCoef out;
    if (m < 1 || !finite_entries(m, a, b)) {
        out.status = TridiagFn::no_convergence;
        return out;
    }
    const int lag = m - std::max(1, m / 8);
    std::vector<double> lagged((size_t)std::max(lag, 1));
    out.status = tridiag_function(m, a, b, fn, param, cj, nullptr, &out.bad);
    if (out.status == TridiagFn::ok && lag > 0) out.status = tridiag_function(lag, a, b, fn, param, lagged.data(), nullptr, &out.bad);
    if (out.status != TridiagFn::ok) return out;
    const double scale = std::sqrt(z2);
    for (int t = 0; t < m; ++t) cj[t] = scale * cj[t];
    double num = 0.0, den = 0.0;
    for (int t = 0; t < m; ++t) {
        const double lt = t < lag ? scale * lagged[t] : 0.0;
        const double d = cj[t] - lt;
        const double d2 = d * d, c2 = cj[t] * cj[t];
        num += d2;
        den += c2;
    }
    out.change = lag == 0 ? 1.0 : den == 0.0 ? 0.0 : std::sqrt(num) / std::sqrt(den);
    return out;
}

}  // namespace

extern "C" {

cgx_status cgx_apply_function(cgx_ctx *ctx, int fn, double param, int nvec, int steps, const double *B, long ldb, double *X, long ldx,
                              int *steps_done, double *change, double *coef)
{
    const std::string name("cgx_apply_function");
    CGX_TRY(check_lanczos(ctx, name, steps));
    if (nvec < 1 || nvec > CGX_MAX_RHS) return fail(ctx, CGX_ERR_BAD_ARG, name + ": nvec must be 1 .. CGX_MAX_RHS");
    if (!B || !X) return fail(ctx, CGX_ERR_BAD_ARG, name + ": null pointer");
    if (ldb < ctx->n || ldx < ctx->n) return fail(ctx, CGX_ERR_BAD_ARG, name + ": leading dimension smaller than n");
    if (fn < CGX_FN_SQRT || fn > CGX_FN_EXP) return fail(ctx, CGX_ERR_BAD_ARG, name + ": fn must be one of CGX_FN_SQRT .. CGX_FN_EXP");
    if (!funm_args_ok(fn, param)) return fail(ctx, CGX_ERR_BAD_ARG, name + ": param of CGX_FN_EXP must be finite and >= 0");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    FunmView v;
    CGX_TRY(ensure_funm(ctx, name, nvec, steps, &v));

    std::vector<double> alpha((size_t)nvec * steps), beta((size_t)nvec * steps), c((size_t)nvec * steps, 0.0);
    int m[kW];
    double z2[kW];
    CGX_TRY(lanczos_run(ctx, name, false, nvec, steps, B, ldb, 0, alpha.data(), beta.data(), m, z2, v.Q));
    // The columns' coefficients are independent of each other: above kThreadedSteps steps (two O(m^2) sweeps per column, some
    // milliseconds at 256 steps) every column gets a host thread of its own.  The refusals are then made in column order.
    ColumnCoef col[kW];
    auto column = [&](int j) {
        col[j] = column_coefficients(m[j], alpha.data() + (size_t)j * steps, beta.data() + (size_t)j * steps, fn, param, z2[j],
                                     c.data() + (size_t)j * steps);
    };
    if (nvec > 1 && steps >= kThreadedSteps) {
        std::vector<std::thread> pool;
        pool.reserve((size_t)nvec);
        for (int j = 1; j < nvec; ++j) {
            try {
                pool.emplace_back(column, j);
            } catch (const std::system_error &) {              // no thread to be had: this one does the column
                column(j);
            }
        }
        column(0);
        for (std::thread &t : pool) t.join();
    } else {
        for (int j = 0; j < nvec; ++j) column(j);
    }
    for (int j = 0; j < nvec; ++j) {
        if (col[j].status == TridiagFn::domain)
            return fail(ctx, CGX_ERR_BAD_ARG, name + ": matrix is not positive definite (Ritz value " + std::to_string(col[j].bad) +
                                                  " from column " + std::to_string(j) + ")");
        if (col[j].status != TridiagFn::ok)
            return fail(ctx, CGX_ERR_BAD_ARG, name + ": the Lanczos coefficients of column " + std::to_string(j) +
                                                  " are not finite, or their Jacobi matrix has no eigen-decomposition");
    }
    CGX_TRY(run_combine(ctx, v, nvec, steps, c.data(), m, X, ldx));
    for (int j = 0; j < nvec; ++j) {
        if (steps_done) steps_done[j] = m[j];
        if (change) change[j] = col[j].change;
    }
    if (coef) std::copy(c.begin(), c.end(), coef);
    return CGX_OK;
}

// TEST PROBE: the combine kernel by itself on a caller's basis Q[((size_t)t * nvec + j) * ldq + i] and coefficients C (nvec rows of
// `steps`), through the side block of cgx_apply_function at the problem's own row pitch.
cgx_status cgx_probe_funm_combine(cgx_ctx *ctx, int nvec, int steps, const int *m, const double *Q, long ldq, const double *C, double *X,
                                  long ldx)
{
    const std::string name("cgx_probe_funm_combine");
    CGX_TRY(check_dense_one_gpu(ctx, name));
    if (nvec < 1 || nvec > CGX_MAX_RHS || steps < 1 || steps > CGX_MAX_LANCZOS_STEPS || !m || !Q || !C || !X || ldq < ctx->n || ldx < ctx->n)
        return fail(ctx, CGX_ERR_BAD_ARG, name + ": bad argument");
    for (int j = 0; j < nvec; ++j)
        if (m[j] < 0 || m[j] > steps) return fail(ctx, CGX_ERR_BAD_ARG, name + ": m must be 0 .. steps");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    FunmView v;
    CGX_TRY(ensure_funm(ctx, name, nvec, steps, &v));
    CGX_TRY(upload_columns(ctx, v.Q, Q, ldq, (size_t)steps * nvec));
    return run_combine(ctx, v, nvec, steps, C, m, X, ldx);
}

}  // extern "C"
