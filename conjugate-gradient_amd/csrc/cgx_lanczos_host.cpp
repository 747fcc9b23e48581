// cgx_lanczos_host.cpp -- cgx_lanczos, cgx_trace_slq, cgx_tridiag_quadrature and cgx_tridiag_function: the host side of the
// multi-vector Lanczos recurrence (cgx_lanczos.hip), stochastic Lanczos quadrature on top of it and the
// host-only functions of a Jacobi matrix (f(T) e_1 for cgx_apply_function).
//
// One GPU, dense storage.  The blocks live in ONE device allocation of the context (cgx_ctx::lanczos), apart from the single
// path's buffers and from the multi blocks, made on the first call of a problem and freed with it.  A step is two launches -- the
// plain multi-vector K1 of cgx_multi.hip as it is, then k_lanczos_step -- and nothing is polled: the steps are queued behind each
// other and one synchronisation ends them.
#include "cgx_internal.h"

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

using namespace cgxi;

namespace {

constexpr int kW = cgx::kMaxRhs;
constexpr int kSlqBatch = 8;   // probes per Lanczos run: the width at which K1m is cheapest per column

struct LanczosView {
    double *V[2], *Y;               // kW x lda each (column j at + j * lda)
    double *k1p;                    // kW x k1p_stride(n): K1m's w.Aw partials
    double *wwp[2];                 // kW x multi_update_grid(n) each: the ||w||^2 partials, ping-pong over the steps
    double *alpha, *beta;           // kW x kMaxLanczosSteps each: the histories
    cgx::LanczosScalars *ls;
};

size_t lanczos_layout(const cgx_ctx *ctx, double *base, LanczosView *v)
{
    const size_t vec = (size_t)kW * ctx->lda;
    Carver c{base};
    v->V[0] = c.take(vec);
    v->V[1] = c.take(vec);
    v->Y = c.take(vec);
    v->k1p = c.take((size_t)kW * k1p_stride(ctx->n));
    v->wwp[0] = c.take((size_t)kW * cgx::multi_update_grid(ctx->n));
    v->wwp[1] = c.take((size_t)kW * cgx::multi_update_grid(ctx->n));
    v->alpha = c.take((size_t)kW * cgx::kMaxLanczosSteps);
    v->beta = c.take((size_t)kW * cgx::kMaxLanczosSteps);
    v->ls = c.take_struct<cgx::LanczosScalars>();
    return c.bytes();
}

}  // namespace

// The checks every entry point on the plain recurrence makes, in this order: context, problem, transport, storage, preconditioner,
// steps.
cgx_status cgxi::check_lanczos(cgx_ctx *ctx, const char *name, int steps)
{
    const std::string fn(name);
    CGX_TRY(check_one_gpu_call(ctx, fn));
    if (ctx->sparse()) return fail(ctx, CGX_ERR_UNSUPPORTED, fn + ": dense storage only (CGX_MATRIX_DENSE)");
    if (ctx->precond != CGX_PRECOND_NONE)
        return fail(ctx, CGX_ERR_UNSUPPORTED, fn + ": a preconditioner is set and would be ignored (cgx_set_preconditioner)");
    if (steps < 1 || steps > CGX_MAX_LANCZOS_STEPS || steps > ctx->n)
        return fail(ctx, CGX_ERR_BAD_ARG, fn + ": steps must be 1 .. min(n, CGX_MAX_LANCZOS_STEPS)");
    return CGX_OK;
}

// THE recurrence: nvec start vectors (one per row of V0, pitch ldv) through `steps` steps.  alpha, beta: nvec rows of `steps`
// doubles, zero at t >= m[j]; z2[j] = ||V0_j||^2 as the device summed it.  col0: the number of row 0 in the caller's own count,
// for the message about a bad start vector.  basis != nullptr (cgx_apply_function): behind step t the block that now holds the
// normalised v_t is copied into slot t of the basis, nvec * lda doubles each; with a null pointer no such call is made.
cgx_status cgxi::lanczos_run(cgx_ctx *ctx, const char *name, int nvec, int steps, const double *V0, long ldv, int col0, double *alpha,
                             double *beta, int *m, double *z2, double *basis)
{
    LanczosView v;
    CGX_TRY(ensure_side_block(ctx, &ctx->lanczos, &ctx->lanczos_bytes, lanczos_layout(ctx, nullptr, &v)));
    lanczos_layout(ctx, ctx->lanczos, &v);
    hipStream_t st = ctx->stream;
    const int n = ctx->n;
    const long lda = ctx->lda;
    const int g1 = cgx::multi_gemv_grid(n, cgx::multi_width(nvec));

    HIP_TRY(ctx, hipMemcpy2DAsync(v.V[0], (size_t)lda * sizeof(double), V0, (size_t)ldv * sizeof(double), (size_t)n * sizeof(double), nvec,
                                  hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, cgx::launch_lanczos_init(n, lda, nvec, v.V[0], v.V[1], v.wwp[0], v.ls, st));
    for (int t = 0; t < steps; ++t) {
        double *w = v.V[t & 1], *vprev = v.V[(t + 1) & 1];
        cgx::MultiArgs g{};
        g.A = ctx->shards[0].A;
        g.lda = lda;
        g.n = n;
        g.nrhs = nvec;
        g.v = w;
        g.Y = v.Y;
        g.partials = v.k1p;
        HIP_TRY(ctx, cgx::launch_multi_gemv(g, false, st));
        cgx::LanczosArgs a{};
        a.n = n;
        a.nvec = nvec;
        a.lda = lda;
        a.w = w;
        a.vprev = vprev;
        a.Y = v.Y;
        a.k1p = v.k1p;
        a.g1 = g1;
        a.ww_in = v.wwp[t & 1];
        a.ww_out = v.wwp[(t + 1) & 1];
        a.ls = v.ls;
        a.alpha = v.alpha;
        a.beta = v.beta;
        a.t = t;
        HIP_TRY(ctx, cgx::launch_lanczos_step(a, st));
        if (basis)
            HIP_TRY(ctx, hipMemcpyAsync(basis + (size_t)t * nvec * lda, w, (size_t)nvec * lda * sizeof(double), hipMemcpyDeviceToDevice, st));
    }
    HIP_TRY(ctx, cgx::launch_lanczos_close(n, nvec, steps, v.wwp[steps & 1], v.ls, v.beta, st));
    cgx::LanczosScalars hs;
    HIP_TRY(ctx, hipMemcpyAsync(&hs, v.ls, sizeof hs, hipMemcpyDeviceToHost, st));
    const size_t row = (size_t)steps * sizeof(double), pitch = (size_t)cgx::kMaxLanczosSteps * sizeof(double);
    HIP_TRY(ctx, hipMemcpy2DAsync(alpha, row, v.alpha, pitch, row, nvec, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpy2DAsync(beta, row, v.beta, pitch, row, nvec, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));

    for (int j = 0; j < nvec; ++j)
        if (hs.bad[j])
            return fail(ctx, CGX_ERR_BAD_ARG, std::string(name) + ": start vector " + std::to_string(col0 + j) + " has norm 0 or is not finite");
    for (int j = 0; j < nvec; ++j) {
        m[j] = hs.m[j];
        z2[j] = hs.z2[j];
        for (int t = m[j]; t < steps; ++t) alpha[(size_t)j * steps + t] = beta[(size_t)j * steps + t] = 0.0;
    }
    return CGX_OK;
}

namespace {

// sqrt(a^2 + b^2) without overflow (the QL sweep's plane rotations)
double pythag(double a, double b) { return std::hypot(a, b); }

// Implicit symmetric QL with Wilkinson's shift on (d, e), carrying the FIRST ROW z of the eigenvector matrix along: the rotations
// of a sweep are applied to z alone, so the work is O(m^2) and nothing m x m is held.  e[i] couples i and i + 1; e[m-1] is work space.
// rec != nullptr: every plane rotation applied to z is appended, in the order applied (about 1.1 m^2 of them); the arithmetic of
// the sweep is the same with and without.
struct Rotation {
    int i;
    double c, s;
};

bool ql_first_row(int m, double *d, double *e, double *z, std::vector<Rotation> *rec = nullptr)
{
    for (int l = 0; l < m; ++l) {
        int iter = 0, mm;
        do {
            for (mm = l; mm < m - 1; ++mm) {
                const double dd = std::fabs(d[mm]) + std::fabs(d[mm + 1]);
                if (std::fabs(e[mm]) + dd == dd) break;
            }
            if (mm != l) {
                if (iter++ == 60) return false;
                double g = (d[l + 1] - d[l]) / (2.0 * e[l]);
                double r = pythag(g, 1.0);
                g = d[mm] - d[l] + e[l] / (g + std::copysign(r, g));
                double s = 1.0, c = 1.0, p = 0.0;
                int i;
                for (i = mm - 1; i >= l; --i) {
                    double f = s * e[i];
                    const double b = c * e[i];
                    r = pythag(f, g);
                    e[i + 1] = r;
                    if (r == 0.0) {
                        d[i + 1] -= p;
                        e[mm] = 0.0;
                        break;
                    }
                    s = f / r;
                    c = g / r;
                    g = d[i + 1] - p;
                    r = (d[i] - g) * s + 2.0 * c * b;
                    p = s * r;
                    d[i + 1] = g + p;
                    g = c * r - b;
                    f = z[i + 1];
                    z[i + 1] = s * z[i] + c * f;
                    z[i] = c * z[i] - s * f;
                    if (rec) rec->push_back(Rotation{i, c, s});
                }
                if (r == 0.0 && i >= l) continue;
                d[l] -= p;
                e[l] = g;
                e[mm] = 0.0;
            }
        } while (mm != l);
    }
    return true;
}

// nodes ascending and weights of the m-point rule; the scratch vectors are the caller's so that a batch allocates once
bool gauss_rule(int m, const double *alpha, const double *beta, double *theta, double *weight, std::vector<double> &work, std::vector<int> &idx)
{
    work.assign((size_t)3 * m, 0.0);
    idx.resize((size_t)m);
    double *d = work.data(), *e = d + m, *z = e + m;
    for (int i = 0; i < m; ++i) {
        d[i] = alpha[i];
        if (i + 1 < m) e[i] = beta[i];
        idx[i] = i;
    }
    z[0] = 1.0;
    if (!ql_first_row(m, d, e, z)) return false;
    std::sort(idx.begin(), idx.end(), [&](int a, int b) { return d[a] < d[b] || (d[a] == d[b] && a < b); });
    for (int i = 0; i < m; ++i) {
        theta[i] = d[idx[i]];
        weight[i] = z[idx[i]] * z[idx[i]];
    }
    return true;
}

// The Rademacher sign of element i of library probe j (include/cgx.h): the top bit of a counter-based hash.
double rademacher(unsigned long long seed_mixed, unsigned long long j, unsigned long long i)
{
    return (cgx::hash_mix64(seed_mixed ^ ((j << 32) | i)) >> 63) ? -1.0 : 1.0;
}

bool funm_in_domain(int fn, double theta)
{
    return fn == CGX_FN_EXP || (fn == CGX_FN_SQRT ? theta >= 0.0 : theta > 0.0);
}

double funm_value(int fn, double param, double theta)
{
    switch (fn) {
    case CGX_FN_SQRT: return std::sqrt(theta);
    case CGX_FN_INVSQRT: return 1.0 / std::sqrt(theta);
    case CGX_FN_INV: return 1.0 / theta;
    case CGX_FN_LOG: return std::log(theta);
    default: return std::exp(-param * theta);
    }
}

}  // namespace

bool cgxi::funm_args_ok(int fn, double param)
{
    if (fn < CGX_FN_SQRT || fn > CGX_FN_EXP) return false;
    return fn != CGX_FN_EXP || (std::isfinite(param) && param >= 0.0);
}

// coef = f(T) e_1 for the m x m Jacobi matrix (alpha, beta), entries and arguments already checked.  The sweep of the Gauss rule runs
// on (d, e, z) with every rotation recorded: with S their product in the order applied, T = S diag(d) S^T and z = S^T e_1, so
// f(T) e_1 = S g with g_k = f(d_k) z_k, and S g is the recorded rotations applied to g from the last one back.  minmax (may be
// null): the smallest and largest d, filled before the domain is looked at.  *bad: the smallest d when it lies outside the domain.
cgxi::TridiagFn cgxi::tridiag_function(int m, const double *alpha, const double *beta, int fn, double param, double *coef, double *minmax,
                                       double *bad)
{
    std::vector<double> work((size_t)3 * m, 0.0);
    std::vector<Rotation> rot;
    rot.reserve((size_t)m * m + (size_t)m * m / 4 + 64);
    double *d = work.data(), *e = d + m, *z = e + m;
    for (int i = 0; i < m; ++i) {
        d[i] = alpha[i];
        if (i + 1 < m) e[i] = beta[i];
    }
    z[0] = 1.0;
    if (!ql_first_row(m, d, e, z, &rot)) return TridiagFn::no_convergence;
    double lo = d[0], hi = d[0];
    for (int i = 1; i < m; ++i) {
        lo = std::min(lo, d[i]);
        hi = std::max(hi, d[i]);
    }
    if (minmax) { minmax[0] = lo; minmax[1] = hi; }
    if (!funm_in_domain(fn, lo)) {
        if (bad) *bad = lo;
        return TridiagFn::domain;
    }
    for (int i = 0; i < m; ++i) coef[i] = funm_value(fn, param, d[i]) * z[i];
    for (size_t r = rot.size(); r-- > 0;) {
        const Rotation &q = rot[r];
        const double a = coef[q.i], b = coef[q.i + 1];
        coef[q.i] = q.c * a + q.s * b;
        coef[q.i + 1] = q.c * b - q.s * a;
    }
    return TridiagFn::ok;
}

// Selected unit eigenvectors of the m x m Jacobi matrix (alpha, beta), entries already checked: the same recorded sweep, T = S diag(d)
// S^T, so the eigenvector of d_k is S e_k -- the recorded rotations applied to e_k from the last one back, O(m^2) each, nothing m x m
// held.  theta (may be null): all eigenvalues ascending (ties by their place in d); index[c] counts in that order; row c of S (m
// doubles) is signed so that its first component is >= 0.  false: no convergence.
bool cgxi::tridiag_eigenvectors(int m, const double *alpha, const double *beta, int nsel, const int *index, double *theta, double *S)
{
    std::vector<double> work((size_t)3 * m, 0.0);
    std::vector<Rotation> rot;
    rot.reserve((size_t)m * m + (size_t)m * m / 4 + 64);
    std::vector<int> idx((size_t)m);
    double *d = work.data(), *e = d + m, *z = e + m;
    for (int i = 0; i < m; ++i) {
        d[i] = alpha[i];
        if (i + 1 < m) e[i] = beta[i];
        idx[i] = i;
    }
    z[0] = 1.0;
    if (!ql_first_row(m, d, e, z, &rot)) return false;
    std::sort(idx.begin(), idx.end(), [&](int a, int b) { return d[a] < d[b] || (d[a] == d[b] && a < b); });
    if (theta)
        for (int i = 0; i < m; ++i) theta[i] = d[idx[i]];
    for (int c = 0; c < nsel; ++c) {
        double *v = S + (size_t)c * m;
        std::fill(v, v + m, 0.0);
        v[idx[index[c]]] = 1.0;
        for (size_t r = rot.size(); r-- > 0;) {
            const Rotation &q = rot[r];
            const double a = v[q.i], b = v[q.i + 1];
            v[q.i] = q.c * a + q.s * b;
            v[q.i + 1] = q.c * b - q.s * a;
        }
        if (v[0] < 0.0)
            for (int i = 0; i < m; ++i) v[i] = -v[i];
    }
    return true;
}

extern "C" {

cgx_status cgx_tridiag_eigenvectors(int m, const double *alpha, const double *beta, int nsel, const int *index, double *theta, double *S)
{
    if (m < 1 || !alpha || !S || (m > 1 && !beta) || nsel < 1 || !index) return CGX_ERR_BAD_ARG;
    for (int i = 0; i < m; ++i)
        if (!std::isfinite(alpha[i]) || (i + 1 < m && !std::isfinite(beta[i]))) return CGX_ERR_BAD_ARG;
    for (int c = 0; c < nsel; ++c)
        if (index[c] < 0 || index[c] >= m) return CGX_ERR_BAD_ARG;
    return tridiag_eigenvectors(m, alpha, beta, nsel, index, theta, S) ? CGX_OK : CGX_ERR_UNSUPPORTED;   // (no convergence in 60 sweeps)
}

cgx_status cgx_tridiag_function(int m, const double *alpha, const double *beta, int fn, double param, double *coef, double *theta_minmax)
{
    if (m < 1 || !alpha || !coef || (m > 1 && !beta) || !funm_args_ok(fn, param)) return CGX_ERR_BAD_ARG;
    for (int i = 0; i < m; ++i)
        if (!std::isfinite(alpha[i]) || (i + 1 < m && !std::isfinite(beta[i]))) return CGX_ERR_BAD_ARG;
    switch (tridiag_function(m, alpha, beta, fn, param, coef, theta_minmax, nullptr)) {
    case TridiagFn::ok: return CGX_OK;
    case TridiagFn::domain: return CGX_ERR_BAD_ARG;        // an eigenvalue where f is not defined (theta_minmax is filled)
    default: return CGX_ERR_UNSUPPORTED;                   // (no convergence in 60 sweeps per value)
    }
}

cgx_status cgx_tridiag_quadrature(int m, const double *alpha, const double *beta, double *theta, double *weight)
{
    if (m < 1 || !alpha || !theta || !weight || (m > 1 && !beta)) return CGX_ERR_BAD_ARG;
    for (int i = 0; i < m; ++i)
        if (!std::isfinite(alpha[i]) || (i + 1 < m && !std::isfinite(beta[i]))) return CGX_ERR_BAD_ARG;
    std::vector<double> e;
    std::vector<int> idx;
    return gauss_rule(m, alpha, beta, theta, weight, e, idx) ? CGX_OK : CGX_ERR_UNSUPPORTED;   // (no convergence in 60 sweeps per value)
}

cgx_status cgx_lanczos(cgx_ctx *ctx, int nvec, int steps, const double *V0, long ldv, double *alpha, double *beta, int *steps_done)
{
    CGX_TRY(check_lanczos(ctx, "cgx_lanczos", steps));
    if (nvec < 1 || nvec > CGX_MAX_RHS) return fail(ctx, CGX_ERR_BAD_ARG, "cgx_lanczos: nvec must be 1 .. CGX_MAX_RHS");
    if (!V0 || !alpha || !beta || !steps_done) return fail(ctx, CGX_ERR_BAD_ARG, "cgx_lanczos: null pointer");
    if (ldv < ctx->n) return fail(ctx, CGX_ERR_BAD_ARG, "cgx_lanczos: leading dimension smaller than n");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    double z2[kW];
    return lanczos_run(ctx, "cgx_lanczos", nvec, steps, V0, ldv, 0, alpha, beta, steps_done, z2);
}

cgx_status cgx_trace_slq(cgx_ctx *ctx, int fn, int nprobe, int steps, unsigned long long seed, const double *Z, long ldz,
                         double *estimate, double *std_error, double *per_probe, double *ritz)
{
    CGX_TRY(check_lanczos(ctx, "cgx_trace_slq", steps));
    if (fn != CGX_SLQ_LOG && fn != CGX_SLQ_INV) return fail(ctx, CGX_ERR_BAD_ARG, "cgx_trace_slq: fn must be CGX_SLQ_LOG or CGX_SLQ_INV");
    if (nprobe < 1 || nprobe > CGX_MAX_PROBES) return fail(ctx, CGX_ERR_BAD_ARG, "cgx_trace_slq: nprobe must be 1 .. CGX_MAX_PROBES");
    if (!estimate || !std_error) return fail(ctx, CGX_ERR_BAD_ARG, "cgx_trace_slq: null pointer");
    if (Z && ldz < ctx->n) return fail(ctx, CGX_ERR_BAD_ARG, "cgx_trace_slq: leading dimension smaller than n");
    HIP_TRY(ctx, hipSetDevice(ctx->device));

    const int n = ctx->n;
    const unsigned long long sm = cgx::hash_mix64(seed);
    std::vector<double> block, value((size_t)nprobe), alpha((size_t)kSlqBatch * steps), beta((size_t)kSlqBatch * steps);
    std::vector<double> theta((size_t)steps), weight((size_t)steps), scratch;
    std::vector<int> idx;
    if (!Z) block.resize((size_t)kSlqBatch * n);
    double lo = HUGE_VAL, hi = -HUGE_VAL;
    for (int j0 = 0; j0 < nprobe; j0 += kSlqBatch) {
        const int nb = std::min(kSlqBatch, nprobe - j0);
        if (!Z)
            for (int j = 0; j < nb; ++j)
                for (int i = 0; i < n; ++i) block[(size_t)j * n + i] = rademacher(sm, (unsigned long long)(j0 + j), (unsigned long long)i);
        int m[kSlqBatch];
        double z2[kSlqBatch];
        CGX_TRY(lanczos_run(ctx, "cgx_trace_slq", nb, steps, Z ? Z + (size_t)j0 * ldz : block.data(), Z ? ldz : (long)n, j0, alpha.data(),
                            beta.data(), m, z2));
        for (int j = 0; j < nb; ++j) {
            const double *a = alpha.data() + (size_t)j * steps, *b = beta.data() + (size_t)j * steps;
            bool finite = m[j] >= 1;
            for (int t = 0; t < m[j] && finite; ++t) finite = std::isfinite(a[t]) && (t + 1 >= m[j] || std::isfinite(b[t]));
            if (!finite || !gauss_rule(m[j], a, b, theta.data(), weight.data(), scratch, idx))
                return fail(ctx, CGX_ERR_BAD_ARG, "cgx_trace_slq: the Lanczos coefficients of probe " + std::to_string(j0 + j) +
                                                      " are not finite, or their Jacobi matrix has no eigen-decomposition");
            if (!(theta[0] > 0.0))
                return fail(ctx, CGX_ERR_BAD_ARG, "cgx_trace_slq: matrix is not positive definite (Ritz value " + std::to_string(theta[0]) +
                                                      " from probe " + std::to_string(j0 + j) + ")");
            double q = 0.0;
            for (int i = 0; i < m[j]; ++i) q += weight[i] * (fn == CGX_SLQ_LOG ? std::log(theta[i]) : 1.0 / theta[i]);   // ascending theta
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

}  // extern "C"
