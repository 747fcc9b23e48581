// cgx_multi.hip -- several right-hand sides against one dense matrix on one GPU (cgx_solve_multi, cgx_probe_gemv_multi).
//
// k independent copies of the single-vector recurrence (cgx_kernels.hip, cg.cc:96-137), one per column of a k-wide block of
// vectors, held column-major at pitch lda: column j of a block is base + j * lda.  Two kernels per iteration, as in the single
// path:
//
//   K1m fused   per column j: rsnew_j = fixed-order fold of K3m's r.r partials; break test; beta_j; p_j = r_j + beta_j p_j
//               (formed while the P tile is staged, stored once) -- then Y = A P with ONE pass over A for all k columns, and
//               one p_j.Ap_j partial per workgroup and column
//   K3m         per live column: p.Ap from K1m's partials in a fixed order, alpha_j, x_j += alpha_j p_j, r_j -= alpha_j Ap_j,
//               the r.r partials of the next head
//
// A column whose break test passes is frozen: no later kernel writes its x, r, p or scalars; the others go on.  Columns
// j >= nrhs of a kernel width (k = 3 runs the 4-wide kernels) are masked by nrhs, never by their values.
//
// The K1m shape and its sum orders: cgx_multi_gemv.inc (the body is shared with the preconditioned form, cgx_multi_pc.hip).
#include "cgx_kernels.h"
#include "cgx_device.h"

#include <hip/hip_ext.h>

namespace cgx {

namespace {

// K1m: the body is cgx_multi_gemv.inc with PRE = false (the plain head: one partial set per column).
template <int W, bool FUSED>
__global__ __launch_bounds__(kMultiThreads, 2) void k_multi_gemv(const double *__restrict__ A, long lda, int n, int nrhs,
                                                                 const double *__restrict__ v, double *__restrict__ p_new,
                                                                 const double *__restrict__ r, const double *__restrict__ rrp,
                                                                 int g3, double *__restrict__ Y, double *__restrict__ partials,
                                                                 MultiScalars *ms, int k, double tol)
{
    constexpr bool PRE = false;
    constexpr const double *rzp = nullptr;
    constexpr MultiPcScalars *mp = nullptr;
#include "cgx_multi_gemv.inc"
}

// K3m: workgroup (b, j) = rows [256 b, 256 b + 256) of column j.  p.Ap = fold of K1m's g1 partials of column j in K3's order,
// alpha_j (cg.cc:107), x += alpha p (cg.cc:110), r -= alpha Ap (cg.cc:113), one r.r partial per workgroup (cg.cc:116).
__global__ __launch_bounds__(256) void k_multi_update(int n, long lda, const double *__restrict__ p, const double *__restrict__ Y,
                                                      const double *__restrict__ partials, int g1, double *__restrict__ x,
                                                      double *__restrict__ r, double *__restrict__ rrp, MultiScalars *ms,
                                                      int parity)
{
    __shared__ double lds[4];
    const int j = blockIdx.y;
    const int done = ms->done[j];
    const double rsold = ms->rs[j][parity];
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const long off = (long)j * lda + i;
    const bool in = i < n;
    double ap_i = 0.0, r_i = 0.0, p_i = 0.0, x_i = 0.0;
    if (in) { ap_i = Y[off]; r_i = r[off]; p_i = p[off]; x_i = x[off]; }
    const double cs = fold_pap(partials + (long)j * g1, 1, 0, g1);
    if (done) return;                                      // frozen column (uniform over the workgroup)
    const double conj = block_sum<4>(cs, lds);
    const double alpha = safeguarded_alpha(rsold, conj);
    double rr = 0.0;
    if (in) {
        const double rn = fma(-alpha, ap_i, r_i);
        r[off] = rn;
        rr = rn * rn;
        x[off] = fma(alpha, p_i, x_i);
    }
    rr = block_sum<4>(rr, lds);
    if (threadIdx.x == 0) rrp[(long)j * gridDim.x + blockIdx.x] = rr;
}

// r_j = b_j - Y_j (Y = A X0, cg.cc:79-82) and its r.r partials (cg.cc:85,91); grid (g3, nrhs).
__global__ __launch_bounds__(256) void k_multi_init(int n, long lda, const double *__restrict__ b, const double *__restrict__ Y,
                                                    double *__restrict__ r, double *__restrict__ rrp)
{
    __shared__ double lds[4];
    const int j = blockIdx.y;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    double rr = 0.0;
    if (i < n) {
        const long off = (long)j * lda + i;
        const double rv = b[off] - Y[off];
        r[off] = rv;
        rr = rv * rv;
    }
    rr = block_sum<4>(rr, lds);
    if (threadIdx.x == 0) rrp[(long)j * gridDim.x + blockIdx.x] = rr;
}

// The loop ran out after k iterations: the head of iteration k for every column (what the next K1m would have done).
__global__ __launch_bounds__(kMultiThreads) void k_multi_close(MultiScalars *ms, const double *__restrict__ rrp, int g3, int nrhs,
                                                               int k, double tol)
{
    const int w = threadIdx.x >> 6;
    for (int j = w; j < nrhs; j += kMultiWaves) {
        double beta;
        (void)multi_head<false>(ms, nullptr, nullptr, rrp, g3, j, k, tol, true, &beta);
    }
}

// Per column j (one workgroup each): ||Y_j + sigma_j x_j - b_j||^2, ||b_j||^2, ||x_j||^2 (cg.cc:146-151) in a fixed order; Y_j =
// A x_j, b_j = b + j * ldb.  SHIFTED = false has no sigma term at all: fma(0, x, Y) is not Y where x is not finite.
template <bool SHIFTED>
__global__ __launch_bounds__(1024) void k_column_norms(int n, long lda, const double *__restrict__ Y, const double *__restrict__ X,
                                                       const double *__restrict__ b, long ldb, ColumnSigmas sg,
                                                       double *__restrict__ norms)
{
    __shared__ double lds[3][16];
    const int j = blockIdx.x;
    const double sig = sg.v[j];
    b += (long)j * ldb;
    double e = 0.0, bb = 0.0, xx = 0.0;
    for (long i = threadIdx.x; i < n; i += 1024) {
        const long off = (long)j * lda + i;
        const double bi = b[i], xi = X[off], d = SHIFTED ? fma(sig, xi, Y[off]) - bi : Y[off] - bi;
        e += d * d;
        bb += bi * bi;
        xx += xi * xi;
    }
    e = wave_sum(e);
    bb = wave_sum(bb);
    xx = wave_sum(xx);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) {
        lds[0][w] = e;
        lds[1][w] = bb;
        lds[2][w] = xx;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        double s = lds[threadIdx.x][0];
        for (int t = 1; t < 16; ++t) s += lds[threadIdx.x][t];
        norms[3 * j + threadIdx.x] = s;
    }
}

template <int W>
hipError_t launch_width(const MultiArgs &g, bool fused, hipStream_t s, hipEvent_t e0, hipEvent_t e1)
{
    const int grid = multi_gemv_grid(g.n, W);
    if (fused)
        hipExtLaunchKernelGGL((k_multi_gemv<W, true>), dim3(grid), dim3(kMultiThreads), 0, s, e0, e1, 0, g.A, g.lda, g.n, g.nrhs, g.v,
                              g.p_new, g.r, g.rrp, multi_update_grid(g.n), g.Y, g.partials, g.ms, g.k, g.tol);
    else
        hipExtLaunchKernelGGL((k_multi_gemv<W, false>), dim3(grid), dim3(kMultiThreads), 0, s, e0, e1, 0, g.A, g.lda, g.n, g.nrhs, g.v,
                              nullptr, nullptr, nullptr, 0, g.Y, g.partials, g.ms, 0, 0.0);
    return hipGetLastError();
}

}  // namespace

int multi_width(int nrhs)
{
    int w = 1;
    while (w < nrhs) w *= 2;
    return w;
}

int multi_rows_per_wg(int width)
{
    switch (width) {
    case 1: return kMultiWaves * MultiShape<1>::R;
    case 2: return kMultiWaves * MultiShape<2>::R;
    case 4: return kMultiWaves * MultiShape<4>::R;
    case 8: return kMultiWaves * MultiShape<8>::R;
    default: return kMultiWaves * MultiShape<16>::R;
    }
}

int multi_gemv_grid(int n, int width) { return (n + multi_rows_per_wg(width) - 1) / multi_rows_per_wg(width); }
int multi_update_grid(int n) { return (n + 255) / 256; }

hipError_t launch_multi_gemv(const MultiArgs &g, bool fused, hipStream_t s, hipEvent_t e0, hipEvent_t e1)
{
    if (g.nrhs < 1 || g.nrhs > kMaxRhs || g.n < 1) return hipErrorInvalidValue;
    return for_multi_width(g.nrhs, [&](auto w) { return launch_width<decltype(w)::value>(g, fused, s, e0, e1); });
}

hipError_t launch_multi_update(int n, long lda, int nrhs, const double *p, const double *Y, const double *partials, int g1, double *x,
                               double *r, double *rrp, MultiScalars *ms, int parity, hipStream_t s)
{
    hipLaunchKernelGGL(k_multi_update, dim3(multi_update_grid(n), nrhs), dim3(256), 0, s, n, lda, p, Y, partials, g1, x, r, rrp, ms,
                       parity);
    return hipGetLastError();
}

hipError_t launch_multi_init(int n, long lda, int nrhs, const double *b, const double *Y, double *r, double *rrp, hipStream_t s)
{
    hipLaunchKernelGGL(k_multi_init, dim3(multi_update_grid(n), nrhs), dim3(256), 0, s, n, lda, b, Y, r, rrp);
    return hipGetLastError();
}

hipError_t launch_multi_close(MultiScalars *ms, const double *rrp, int n, int nrhs, int k, double tol, hipStream_t s)
{
    hipLaunchKernelGGL(k_multi_close, dim3(1), dim3(kMultiThreads), 0, s, ms, rrp, multi_update_grid(n), nrhs, k, tol);
    return hipGetLastError();
}

hipError_t launch_column_norms(int n, long lda, int ncol, const double *Y, const double *X, const double *b, long ldb,
                               const double *sigma, double *norms, hipStream_t s)
{
    if (ncol < 1 || ncol > kMaxRhs || n < 1 || lda < n) return hipErrorInvalidValue;
    if (sigma)
        hipLaunchKernelGGL(k_column_norms<true>, dim3(ncol), dim3(1024), 0, s, n, lda, Y, X, b, ldb, column_sigmas(sigma, ncol), norms);
    else
        hipLaunchKernelGGL(k_column_norms<false>, dim3(ncol), dim3(1024), 0, s, n, lda, Y, X, b, ldb, ColumnSigmas{}, norms);
    return hipGetLastError();
}

}  // namespace cgx
