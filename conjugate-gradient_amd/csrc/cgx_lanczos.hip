// cgx_lanczos.hip -- the update kernels of the multi-vector Lanczos recurrence (cgx_lanczos, cgx_trace_slq).
//
// Per column j of a block of up to kMaxRhs vectors (column-major at pitch lda, as cgx_multi.hip):
//
//   v_0 = V0_j / ||V0_j||, v_-1 = 0
//   step t:  y = A v_t;  alpha_t = v_t . y;  w = y - alpha_t v_t - beta_(t-1) v_(t-1);  beta_t = ||w||;  v_(t+1) = w / beta_t
//
// The mat-vec is the plain multi-vector K1 (cgx_multi.hip, untouched), run on the NOT YET NORMALISED w_t: it leaves Y = A w_t and
// the partials of w_t . A w_t.  k_lanczos_step then does the rest of step t in one launch: beta_(t-1) = sqrt of the ||w_t||^2
// partials the previous step left, the breakdown test, alpha_t = (w_t . A w_t) / ||w_t||^2, and per row v = w / beta, y = Y / beta,
// w' = y - alpha v - beta v_prev; v goes over w, w' over v_prev (each element belongs to one thread), and the workgroup leaves one
// ||w'||^2 partial.  The host swaps the two blocks between steps.
//
// Every workgroup of a column folds the same partials in the same fixed order (fold_pap + block_sum<4>) and so takes the same
// decision; workgroup (0, j) alone writes the column's scalars and histories, with plain stores.  A frozen column has nothing
// written any more.  No floating-point atomics; no sum depends on the column's position in the block.
#include "cgx_kernels.h"
#include "cgx_device.h"

namespace cgx {

namespace {

constexpr double kLanczosBreak = 0x1.0p-36;   // beta_t <= 2^-36 max |alpha|: an invariant subspace

__global__ __launch_bounds__(1024) void k_lanczos_init(int n, long lda, const double *__restrict__ w, double *__restrict__ vprev,
                                                       double *__restrict__ ww, int g3, LanczosScalars *ls)
{
    __shared__ double lds[16];
    const int j = blockIdx.x;
    double s = 0.0;
    for (long i = threadIdx.x; i < n; i += 1024) {
        const long off = (long)j * lda + i;
        const double wi = w[off];
        s = fma(wi, wi, s);
        vprev[off] = 0.0;
    }
    s = wave_sum(s);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) lds[wv] = s;
    __syncthreads();
    double tot = lds[0];
    for (int u = 1; u < 16; ++u) tot += lds[u];
    for (int b = threadIdx.x; b < g3; b += 1024) ww[(long)j * g3 + b] = b == 0 ? tot : 0.0;   // the column's one partial
    if (threadIdx.x == 0) {
        const bool ok = tot > 0.0 && tot <= 1.7976931348623157e308;   // false for 0, inf and NaN
        ls->amax[j][0] = 0.0;
        ls->amax[j][1] = 0.0;
        ls->z2[j] = tot;
        ls->m[j] = ok ? kLanczosLive : -1;
        ls->bad[j] = ok ? 0 : 1;
    }
}

// Workgroup (b, j) = rows [256 b, 256 b + 256) of column j.
__global__ __launch_bounds__(256) void k_lanczos_step(int n, long lda, double *__restrict__ w, double *__restrict__ vprev,
                                                      const double *__restrict__ Y, const double *__restrict__ k1p, int g1,
                                                      const double *__restrict__ ww_in, double *__restrict__ ww_out,
                                                      LanczosScalars *ls, double *__restrict__ ha, double *__restrict__ hb, int t)
{
    __shared__ double lds[4];
    const int j = blockIdx.y;
    const int g3 = gridDim.x;
    const int mj = ls->m[j];
    const double amax = ls->amax[j][t & 1];
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const long off = (long)j * lda + i;
    const bool in = i < n;
    double w_i = 0.0, y_i = 0.0, u_i = 0.0;
    if (in) { w_i = w[off]; y_i = Y[off]; u_i = vprev[off]; }
    const double ws = fold_pap(ww_in + (long)j * g3, 1, 0, g3);
    const double cs = fold_pap(k1p + (long)j * g1, 1, 0, g1);
    if (mj < t) return;                                    // frozen in an earlier step (uniform: only step mj writes mj)
    const double ww = block_sum<4>(ws, lds);               // ||w_t||^2
    const double wAw = block_sum<4>(cs, lds);              // w_t . A w_t
    const double beta = sqrt(ww);                          // beta_(t-1); t = 0: ||V0_j||
    const bool writer = blockIdx.x == 0 && threadIdx.x == 0;
    const long h = (long)j * kMaxLanczosSteps + t;
    if (writer && t > 0) hb[h - 1] = beta;
    if (beta <= kLanczosBreak * amax) {                    // breakdown: the column is frozen with m = t
        if (writer) ls->m[j] = t;
        return;
    }
    const double alpha = wAw / ww;
    if (writer) {
        ha[h] = alpha;
        const double aa = fabs(alpha);
        ls->amax[j][(t + 1) & 1] = aa > amax ? aa : amax;
    }
    double nw = 0.0;
    if (in) {
        const double v = w_i / beta, y = y_i / beta;
        const double wn = fma(-beta, u_i, fma(-alpha, v, y));
        w[off] = v;
        vprev[off] = wn;
        nw = wn * wn;
    }
    nw = block_sum<4>(nw, lds);
    if (threadIdx.x == 0) ww_out[(long)j * g3 + blockIdx.x] = nw;
}

// One workgroup per column: the last beta, and m = steps for a column that ran to the end.
__global__ __launch_bounds__(256) void k_lanczos_close(const double *__restrict__ ww, int g3, int steps, LanczosScalars *ls,
                                                       double *__restrict__ hb)
{
    __shared__ double lds[4];
    const int j = blockIdx.x;
    const int mj = ls->m[j];
    const double ws = fold_pap(ww + (long)j * g3, 1, 0, g3);
    if (mj != kLanczosLive) return;
    const double tot = block_sum<4>(ws, lds);
    if (threadIdx.x == 0) {
        hb[(long)j * kMaxLanczosSteps + steps - 1] = sqrt(tot);
        ls->m[j] = steps;
    }
}

}  // namespace

hipError_t launch_lanczos_init(int n, long lda, int nvec, const double *w, double *vprev, double *ww, LanczosScalars *ls, hipStream_t s)
{
    if (nvec < 1 || nvec > kMaxRhs || n < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_lanczos_init, dim3(nvec), dim3(1024), 0, s, n, lda, w, vprev, ww, multi_update_grid(n), ls);
    return hipGetLastError();
}

hipError_t launch_lanczos_step(const LanczosArgs &a, hipStream_t s)
{
    if (a.nvec < 1 || a.nvec > kMaxRhs || a.n < 1 || a.t < 0 || a.t >= kMaxLanczosSteps) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_lanczos_step, dim3(multi_update_grid(a.n), a.nvec), dim3(256), 0, s, a.n, a.lda, a.w, a.vprev, a.Y, a.k1p, a.g1,
                       a.ww_in, a.ww_out, a.ls, a.alpha, a.beta, a.t);
    return hipGetLastError();
}

hipError_t launch_lanczos_close(int n, int nvec, int steps, const double *ww, LanczosScalars *ls, double *beta, hipStream_t s)
{
    if (nvec < 1 || nvec > kMaxRhs || steps < 1 || steps > kMaxLanczosSteps) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_lanczos_close, dim3(nvec), dim3(256), 0, s, ww, multi_update_grid(n), steps, ls, beta);
    return hipGetLastError();
}

}  // namespace cgx
