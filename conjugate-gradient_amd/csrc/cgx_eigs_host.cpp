// cgx_eigs_host.cpp -- cgx_eigenpairs and its two probes: extreme eigenpairs by Lanczos with full reorthogonalisation (DESIGN.md
// section 20).
//
// One GPU, dense storage, no preconditioner, one start vector.  A step is six launches -- the plain multi-vector K1 of cgx_multi.hip
// at width 1 as it is, then the five kernels of cgx_eigs.hip -- and with tol = 0 nothing is polled: the steps are queued behind each
// other and one synchronisation ends them.  With tol > 0 the host reads alpha and beta behind every 16th step, forms the wanted Ritz
// pairs of T (tridiag_eigenvectors, cgx_tridiag.cpp) and stops once their estimates are small.  The Ritz vectors are one launch
// of k_eigs_combine over the basis, their residuals one more plain K1m on them and k_eigs_residual.  Everything lives in ONE device
// allocation of the context (cgx_ctx::eigs), apart from every other path's buffers.
#include "cgx_internal.h"

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

using namespace cgxi;

namespace {

constexpr int kW = cgx::kMaxRhs;
constexpr int kPollEvery = 16;   // tol > 0: steps between two looks at the Ritz estimates

struct EigsView {
    double *Y, *W;                  // lda each: A q_t and the vector under orthogonalisation
    double *k1p;                    // kW x k1p_stride(n): K1m's partials (the steps use width 1, the residuals that of nev)
    double *hp, *h, *wwp;           // the projection partials, the folded h, the ||w||^2 partials
    double *alpha, *beta;           // kMaxLanczosSteps each
    cgx::EigsScalars *sc;
    double *C;                      // kMaxLanczosSteps x kW: the Ritz coefficients, step-major
    double *X, *YX;                 // kW x lda each: the Ritz vectors and A times them
    double *theta, *rn;             // kW each: the wanted Ritz values, the squared residual norms
    double *Q;                      // (steps + 1) x lda of the call: the basis, last so that the fixed pieces stay where they are
};

size_t eigs_layout(const cgx_ctx *ctx, double *base, int steps, EigsView *v)
{
    const size_t tiles = (size_t)cgx::eigs_tiles(ctx->n);
    Carver c{base};
    v->Y = c.take((size_t)ctx->lda);
    v->W = c.take((size_t)ctx->lda);
    v->k1p = c.take((size_t)kW * k1p_stride(ctx->n));
    v->hp = c.take(tiles * cgx::kEigsSlotPitch);
    v->h = c.take(cgx::kEigsSlotPitch);
    v->wwp = c.take(tiles);
    v->alpha = c.take(cgx::kMaxLanczosSteps);
    v->beta = c.take(cgx::kMaxLanczosSteps);
    v->sc = c.take_struct<cgx::EigsScalars>();
    v->C = c.take((size_t)cgx::kMaxLanczosSteps * kW);
    v->X = c.take((size_t)kW * ctx->lda);
    v->YX = c.take((size_t)kW * ctx->lda);
    v->theta = c.take(kW);
    v->rn = c.take(kW);
    v->Q = c.take(((size_t)steps + 1) * ctx->lda);
    return c.bytes();
}

// The block for a call of `steps`: made on first use, made again when this call needs more than it holds.
cgx_status ensure_eigs(cgx_ctx *ctx, const std::string &fn, int steps, EigsView *v)
{
    CGX_TRY(ensure_growing_block(ctx, &ctx->eigs, &ctx->eigs_bytes, eigs_layout(ctx, nullptr, steps, v), fn,
                                 "8 (steps + 1) lda = " + std::to_string(steps + 1) + " x " + std::to_string(ctx->lda) +
                                     " doubles, and the work vectors"));
    eigs_layout(ctx, ctx->eigs, steps, v);
    return CGX_OK;
}

cgx::EigsArgs step_args(const cgx_ctx *ctx, const EigsView &v, int t)
{
    cgx::EigsArgs a{};
    a.n = ctx->n;
    a.lda = ctx->lda;
    a.t = t;
    a.Q = v.Q;
    a.Y = v.Y;
    a.W = v.W;
    a.k1p = v.k1p;
    a.g1 = cgx::multi_gemv_grid(ctx->n, 1);
    a.hp = v.hp;
    a.h = v.h;
    a.wwp = v.wwp;
    a.alpha = v.alpha;
    a.beta = v.beta;
    a.sc = v.sc;
    return a;
}

// v0 into slot 0 and the set-up kernel behind it.
cgx_status eigs_begin(cgx_ctx *ctx, const EigsView &v, const double *v0)
{
    HIP_TRY(ctx, hipMemcpyAsync(v.Q, v0, (size_t)ctx->n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, cgx::launch_eigs_init(ctx->n, v.Q, v.sc, ctx->stream));
    return CGX_OK;
}

// Steps t0 .. t1 - 1, queued.
cgx_status eigs_steps(cgx_ctx *ctx, const EigsView &v, int t0, int t1)
{
    hipStream_t st = ctx->stream;
    for (int t = t0; t < t1; ++t) {
        HIP_TRY(ctx, cgx::launch_multi_gemv(plain_k1m_args(ctx, 1, v.Q + (size_t)t * ctx->lda, v.Y, v.k1p), false, st));
        const cgx::EigsArgs a = step_args(ctx, v, t);
        HIP_TRY(ctx, cgx::launch_eigs_project(a, true, st));
        HIP_TRY(ctx, cgx::launch_eigs_subtract(a, false, st));
        HIP_TRY(ctx, cgx::launch_eigs_project(a, false, st));
        HIP_TRY(ctx, cgx::launch_eigs_subtract(a, true, st));
        HIP_TRY(ctx, cgx::launch_eigs_normalise(a, st));
    }
    return CGX_OK;
}

// The scalars and the first `count` alpha and beta, behind everything queued so far.  *m: the steps made (count, or fewer when
// the run is frozen), *live: it is not; a bad start vector is refused here.
cgx_status eigs_read(cgx_ctx *ctx, const std::string &fn, const EigsView &v, int count, double *alpha, double *beta, int *m,
                     bool *live = nullptr)
{
    hipStream_t st = ctx->stream;
    cgx::EigsScalars hs;
    HIP_TRY(ctx, hipMemcpyAsync(&hs, v.sc, sizeof hs, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(alpha, v.alpha, (size_t)count * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(beta, v.beta, (size_t)count * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    if (hs.bad) return fail(ctx, CGX_ERR_BAD_ARG, fn + ": the start vector has norm 0 or is not finite");
    *m = hs.m == cgx::kEigsLive ? count : std::min(hs.m, count);
    if (live) *live = hs.m == cgx::kEigsLive;
    return CGX_OK;
}

// The wanted Ritz pairs of the leading m x m block: theta_all ascending (m), and for j < min(nev, m) value[j], the eigenvector
// S[j * m ..] and estimate[j] = beta_(m-1) |last component|.
struct Ritz {
    int nfound = 0;
    double scale = 0.0;             // max |theta| over all Ritz values
    std::vector<double> theta, S;
    double value[kW], estimate[kW];
};

bool ritz_pairs(int m, const double *alpha, const double *beta, int which, int nev, Ritz *r)
{
    for (int t = 0; t < m; ++t)
        if (!std::isfinite(alpha[t]) || !std::isfinite(beta[t])) return false;
    r->nfound = std::min(nev, m);
    r->theta.assign((size_t)m, 0.0);
    r->S.assign((size_t)r->nfound * m, 0.0);
    int index[kW];
    for (int j = 0; j < r->nfound; ++j) index[j] = which == CGX_EIG_LARGEST ? m - 1 - j : j;
    if (!tridiag_eigenvectors(m, alpha, beta, r->nfound, index, r->theta.data(), r->S.data())) return false;
    r->scale = std::max(std::fabs(r->theta[0]), std::fabs(r->theta[(size_t)m - 1]));
    for (int j = 0; j < r->nfound; ++j) {
        r->value[j] = r->theta[(size_t)index[j]];
        r->estimate[j] = beta[m - 1] * std::fabs(r->S[(size_t)j * m + (m - 1)]);
    }
    return true;
}

}  // namespace

extern "C" {

cgx_status cgx_eigenpairs(cgx_ctx *ctx, int which, int nev, int steps, double tol, const double *v0, unsigned long long seed, double *values,
                          double *vectors, long ldv, double *residual, double *estimate, int *steps_done, int *nfound)
{
    const std::string name("cgx_eigenpairs");
    CGX_TRY(check_lanczos(ctx, name, steps));
    if (which != CGX_EIG_LARGEST && which != CGX_EIG_SMALLEST)
        return fail(ctx, CGX_ERR_BAD_ARG, name + ": which must be CGX_EIG_LARGEST or CGX_EIG_SMALLEST");
    if (nev < 1 || nev > CGX_MAX_EIGENPAIRS || nev > steps) return fail(ctx, CGX_ERR_BAD_ARG, name + ": nev must be 1 .. min(steps, CGX_MAX_EIGENPAIRS)");
    if (!(tol >= 0.0) || !std::isfinite(tol)) return fail(ctx, CGX_ERR_BAD_ARG, name + ": tol must be finite and >= 0");
    if (!values) return fail(ctx, CGX_ERR_BAD_ARG, name + ": null pointer");
    if (vectors && ldv < ctx->n) return fail(ctx, CGX_ERR_BAD_ARG, name + ": leading dimension smaller than n");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    EigsView v;
    CGX_TRY(ensure_eigs(ctx, name, steps, &v));

    hipStream_t st = ctx->stream;
    const int n = ctx->n;
    std::vector<double> start;
    if (!v0) {
        const unsigned long long sm = cgx::hash_mix64(seed);
        start.resize((size_t)n);
        for (int i = 0; i < n; ++i) start[(size_t)i] = cgx::rademacher_sign(sm, 0, (unsigned long long)i);   // probe 0 of cgx_trace_slq
    }
    std::vector<double> alpha((size_t)steps), beta((size_t)steps);
    CGX_TRY(eigs_begin(ctx, v, v0 ? v0 : start.data()));
    Ritz rz;
    int t = 0, m = 0;
    bool have_ritz = false;
    while (t < steps) {
        const int t1 = tol > 0.0 ? std::min(steps, (t / kPollEvery + 1) * kPollEvery) : steps;
        CGX_TRY(eigs_steps(ctx, v, t, t1));
        t = t1;
        CGX_TRY(eigs_read(ctx, name, v, t, alpha.data(), beta.data(), &m));
        if (m < 1 || !ritz_pairs(m, alpha.data(), beta.data(), which, nev, &rz))
            return fail(ctx, CGX_ERR_BAD_ARG, name + ": the Lanczos coefficients are not finite, or their Jacobi matrix has no eigen-decomposition");
        have_ritz = true;
        if (m < t) break;                                      // frozen: the later launches would exit at once
        bool small = rz.nfound == nev;
        for (int j = 0; j < rz.nfound; ++j) small = small && rz.estimate[j] <= tol * rz.scale;
        if (tol > 0.0 && small) break;
    }
    if (!have_ritz) return fail(ctx, CGX_ERR_BAD_ARG, name + ": no step was made");
    const int nf = rz.nfound, wd = cgx::multi_width(nf);

    // the Ritz vectors: the coefficients step-major at the kernel's width, one launch over the basis; then A times them and the norms
    std::vector<double> coef((size_t)m * wd, 0.0);
    for (int j = 0; j < nf; ++j)
        for (int s = 0; s < m; ++s) coef[(size_t)s * wd + j] = rz.S[(size_t)j * m + s];
    double rn[kW];
    HIP_TRY(ctx, hipMemcpyAsync(v.C, coef.data(), coef.size() * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(v.theta, rz.value, (size_t)nf * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, cgx::launch_eigs_combine(n, ctx->lda, m, nf, v.Q, v.C, v.X, ctx->lda, st));
    HIP_TRY(ctx, cgx::launch_multi_gemv(plain_k1m_args(ctx, nf, v.X, v.YX, v.k1p), false, st));
    HIP_TRY(ctx, cgx::launch_eigs_residual(n, ctx->lda, nf, v.YX, v.X, v.theta, v.rn, st));
    HIP_TRY(ctx, hipMemcpyAsync(rn, v.rn, (size_t)nf * sizeof(double), hipMemcpyDeviceToHost, st));
    if (vectors) CGX_TRY(download_columns(ctx, vectors, ldv, v.X, nf));
    HIP_TRY(ctx, hipStreamSynchronize(st));

    for (int j = 0; j < nev; ++j) {
        values[j] = j < nf ? rz.value[j] : 0.0;
        if (residual) residual[j] = j < nf ? std::sqrt(rn[j]) : 0.0;
        if (estimate) estimate[j] = j < nf ? rz.estimate[j] : 0.0;
        if (vectors && j >= nf) std::fill(vectors + (size_t)j * ldv, vectors + (size_t)j * ldv + n, 0.0);
    }
    if (steps_done) *steps_done = m;
    if (nfound) *nfound = nf;
    return CGX_OK;
}

// TEST PROBE: the recurrence alone.  Q receives slots 0 .. m - 1 and, when the run was not frozen (then m = steps), slot m, the next
// vector: steps + 1 rows of ldq doubles must be there.
cgx_status cgx_probe_eigs_basis(cgx_ctx *ctx, int steps, const double *v0, double *Q, long ldq, double *alpha, double *beta, int *steps_done)
{
    const std::string name("cgx_probe_eigs_basis");
    CGX_TRY(check_lanczos(ctx, name, steps));
    if (!v0 || !Q || !alpha || !beta || !steps_done) return fail(ctx, CGX_ERR_BAD_ARG, name + ": null pointer");
    if (ldq < ctx->n) return fail(ctx, CGX_ERR_BAD_ARG, name + ": leading dimension smaller than n");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    EigsView v;
    CGX_TRY(ensure_eigs(ctx, name, steps, &v));
    std::vector<double> a((size_t)steps), b((size_t)steps);
    int m = 0;
    bool live = false;
    CGX_TRY(eigs_begin(ctx, v, v0));
    CGX_TRY(eigs_steps(ctx, v, 0, steps));
    CGX_TRY(eigs_read(ctx, name, v, steps, a.data(), b.data(), &m, &live));
    const int rows = live ? steps + 1 : m;
    CGX_TRY(download_columns(ctx, Q, ldq, v.Q, (size_t)rows));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (int t = 0; t < steps; ++t) {
        alpha[t] = t < m ? a[(size_t)t] : 0.0;
        beta[t] = t < m ? b[(size_t)t] : 0.0;
    }
    *steps_done = m;
    return CGX_OK;
}

// TEST PROBE: ONE projection + subtraction pass on the caller's slots (nslots rows of Q) and w.  The slots the call uses, the slot
// behind them and the vector are first filled with NaN bytes over their whole pitch, so that a read of a pad row or of slot nslots
// shows in the result.
cgx_status cgx_probe_eigs_orthogonalise(cgx_ctx *ctx, int nslots, const double *Q, long ldq, const double *w_in, double *w_out, double *h_out)
{
    const std::string name("cgx_probe_eigs_orthogonalise");
    CGX_TRY(check_dense_one_gpu(ctx, name));
    if (nslots < 1 || nslots > CGX_MAX_LANCZOS_STEPS || !Q || !w_in || !w_out || !h_out || ldq < ctx->n)
        return fail(ctx, CGX_ERR_BAD_ARG, name + ": bad argument");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    EigsView v;
    CGX_TRY(ensure_eigs(ctx, name, nslots, &v));
    hipStream_t st = ctx->stream;
    const size_t row = (size_t)ctx->n * sizeof(double), pitch = (size_t)ctx->lda * sizeof(double);
    cgx::EigsScalars hs{};
    hs.m = cgx::kEigsLive;
    HIP_TRY(ctx, hipMemsetAsync(v.Q, 0xFF, ((size_t)nslots + 1) * pitch, st));
    HIP_TRY(ctx, hipMemsetAsync(v.W, 0xFF, pitch, st));
    CGX_TRY(upload_columns(ctx, v.Q, Q, ldq, (size_t)nslots));
    HIP_TRY(ctx, hipMemcpyAsync(v.W, w_in, row, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(v.sc, &hs, sizeof hs, hipMemcpyHostToDevice, st));
    const cgx::EigsArgs a = step_args(ctx, v, nslots - 1);
    HIP_TRY(ctx, cgx::launch_eigs_project(a, false, st));
    HIP_TRY(ctx, cgx::launch_eigs_subtract(a, false, st));
    HIP_TRY(ctx, hipMemcpyAsync(w_out, v.W, row, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(h_out, v.h, (size_t)nslots * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return CGX_OK;
}

}  // extern "C"
