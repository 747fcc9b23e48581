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
// K1m shape: 8 waves per workgroup, each wave owns R consecutive rows, the workgroup 8R.  The workgroup sweeps the columns in
// chunks of kMultiChunk; the chunk of all W vectors is staged in LDS as [column j][kMultiChunk doubles], so that a lane's
// 16-B read of (j, c..c+1) is conflict free across the wave, and every lane streams its R rows of A with one 16-B load per row
// and 128-column step.  Every staged vector element serves the 8R rows of the workgroup; the A stream is the same as K1's.
// Per row and column the sum order is fixed (lane: ascending chunks and steps, .x then .y; wave: wave_sum_rows), and it does
// not depend on the column's position among the others, so permuting the columns permutes the results bit for bit.
#include "cgx_kernels.h"
#include "cgx_device.h"

#include <hip/hip_ext.h>

namespace cgx {

namespace {

constexpr int kMultiWaves = 8;
constexpr int kMultiThreads = kMultiWaves * 64;
constexpr int kMultiChunk = 256;                     // columns staged per chunk (2 steps of 128)
constexpr int kMultiSteps = kMultiChunk / 128;

// rows per wave for a kernel width: R * W <= 32 partial sums per lane; W = 16 takes one row (two spill: the staged P and the
// unrolled LDS reads of 16 columns come on top of the sums)
template <int W>
struct MultiShape {
    static constexpr int R = W <= 4 ? 8 : (W == 8 ? 4 : 1);
};

// Per column j: the head of iteration k (cg.cc:116-132 of iteration k-1) from the r.r partials rrp[j * g3 + 0 .. g3).  Run by
// one wave; every workgroup of the launch folds the same values in the same order, so every workgroup takes the same decision.
// Writes (workgroup 0 only, and nothing for a column that is already frozen): rs, done, k_final.  Returns whether the column
// runs this iteration, and its beta.
__device__ __forceinline__ bool multi_head(MultiScalars *ms, const double *__restrict__ rrp, int g3, int j, int k, double tol,
                                           bool writer, double *beta)
{
    const int lane = threadIdx.x & 63;
    const int done = ms->done[j];
    const double rsold = ms->rs[j][(k > 0 ? k - 1 : 0) & 1];
    const double *part = rrp + (long)j * g3;
    double v = 0.0;
    for (int t = lane; t < g3; t += 256) {
        double a[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int f = t + 64 * u;
            const double val = part[f < g3 ? f : g3 - 1];
            a[u] = f < g3 ? val : 0.0;
        }
        v += (a[0] + a[1]) + (a[2] + a[3]);
    }
    const double rsnew = wave_sum(v);                       // r.r, cg.cc:116-117 (k == 0: cg.cc:91-92)
    *beta = 0.0;
    if (done) return false;                                 // frozen: nothing is written any more
    const bool first = writer && lane == 0;
    if (k == 0) {                                           // p = r (cg.cc:85): beta = 0, p_old = 0
        if (first) { ms->rs[j][0] = rsnew; ms->rs[j][1] = rsnew; }
        return true;
    }
    if (first) ms->rs[j][k & 1] = rsnew;                    // rsold = rsnew, cg.cc:132
    if (sqrt(rsnew) < tol) {                                // cg.cc:120-121: break before the p update
        if (first) { ms->k_final[j] = k - 1; ms->done[j] = 1; }
        return false;
    }
    *beta = rsnew / rsold;                                  // cg.cc:124
    return true;
}

// K1m.  FUSED: iteration head, P = R + beta P_old staged (and stored once: chunk c by workgroup c mod grid), Y = A P, partials.
// Plain: Y = A V for the nrhs columns of V, partials of V_j . Y_j.  Y, partials and p_new are written for live columns only.
template <int W, bool FUSED>
__global__ __launch_bounds__(kMultiThreads, 2) void k_multi_gemv(const double *__restrict__ A, long lda, int n, int nrhs,
                                                                 const double *__restrict__ v, double *__restrict__ p_new,
                                                                 const double *__restrict__ r, const double *__restrict__ rrp,
                                                                 int g3, double *__restrict__ Y, double *__restrict__ partials,
                                                                 MultiScalars *ms, int k, double tol)
{
    constexpr int R = MultiShape<W>::R;
    constexpr int ROWS = kMultiWaves * R;
    constexpr int NV = R * W;
    __shared__ d2 tile[2][W][kMultiChunk / 2];
    __shared__ double red[kMultiWaves][NV];
    __shared__ double s_beta[W];
    __shared__ int s_live[W];

    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // wave-uniform: the row pointers live in SGPRs
    const int tid = threadIdx.x;

    if constexpr (FUSED) {
        for (int j = w; j < W; j += kMultiWaves) {
            double beta = 0.0;
            const bool live = j < nrhs && multi_head(ms, rrp, g3, j, k, tol, blockIdx.x == 0, &beta);
            if (lane == 0) { s_beta[j] = beta; s_live[j] = live ? 1 : 0; }
        }
    } else {
        if (tid < W) { s_beta[tid] = 0.0; s_live[tid] = tid < nrhs ? 1 : 0; }
    }
    __syncthreads();
    int any = 0;
#pragma unroll
    for (int j = 0; j < W; ++j) any |= s_live[j];
    if (FUSED && blockIdx.x == 0 && tid == 0 && !any && !ms->all_done) {
        ms->all_done = 1;                                   // the host polls this word
        ms->k_all = k - 1;
    }
    if (!any) return;                                       // every column has broken: the grid drains at once

    const long row_w = (long)blockIdx.x * ROWS + (long)w * R;
    const char *a_row[R];
#pragma unroll
    for (int i = 0; i < R; ++i) {
        long row = row_w + i;
        if (row > n - 1) row = n - 1;                       // tail workgroup: re-read the last row, result discarded
        a_row[i] = reinterpret_cast<const char *>(A + row * lda);
    }
    double acc[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) acc[i] = 0.0;

    const int ncols = (n + 1) & ~1;                         // pad columns up to lda are zero in A and in every vector
    const int nchunks = (ncols + kMultiChunk - 1) / kMultiChunk;
    constexpr int kStage = (W * kMultiChunk / 2 + kMultiThreads - 1) / kMultiThreads;   // 16-B pieces per thread and chunk
    d2 st[kStage];

    // the staged value of piece q of chunk c: (column j, 2 doubles); zero for a masked column and past n
    auto stage_load = [&](int c) {
#pragma unroll
        for (int u = 0; u < kStage; ++u) {
            const int q = tid + u * kMultiThreads;
            const int j = q / (kMultiChunk / 2), cc = q % (kMultiChunk / 2);
            const long col = (long)c * kMultiChunk + 2 * cc;
            d2 val = {0.0, 0.0};
            if (q < W * kMultiChunk / 2 && col < ncols && s_live[j]) {
                const long off = (long)j * lda + col;
                if constexpr (FUSED) {
                    const d2 po = *reinterpret_cast<const d2 *>(v + off);
                    const d2 rr = *reinterpret_cast<const d2 *>(r + off);
                    val.x = fma(s_beta[j], po.x, rr.x);     // cg.cc:127-129
                    val.y = fma(s_beta[j], po.y, rr.y);
                } else {
                    val = *reinterpret_cast<const d2 *>(v + off);
                }
            }
            st[u] = val;
        }
    };
    auto stage_store = [&](int c, int buf) {
        const bool owner = FUSED && (c % (int)gridDim.x) == (int)blockIdx.x;
#pragma unroll
        for (int u = 0; u < kStage; ++u) {
            const int q = tid + u * kMultiThreads;
            if (q < W * kMultiChunk / 2) {
                const int j = q / (kMultiChunk / 2), cc = q % (kMultiChunk / 2);
                tile[buf][j][cc] = st[u];
                const long col = (long)c * kMultiChunk + 2 * cc;
                if (owner && col < ncols && s_live[j]) *reinterpret_cast<d2 *>(p_new + (long)j * lda + col) = st[u];   // stored once
            }
        }
    };

    stage_load(0);
    stage_store(0, 0);
    __syncthreads();
    for (int c = 0; c < nchunks; ++c) {
        d2 a[kMultiSteps][R];
#pragma unroll
        for (int s = 0; s < kMultiSteps; ++s) {
            const int col = c * kMultiChunk + s * 128 + lane * 2;
            const unsigned off = (unsigned)(col < ncols ? col : 0) * 8u;
#pragma unroll
            for (int i = 0; i < R; ++i) {
                const d2 val = load_a<true>(reinterpret_cast<const double *>(a_row[i] + off));
                a[s][i] = col < ncols ? val : d2{0.0, 0.0};
            }
        }
        if (c + 1 < nchunks) stage_load(c + 1);
        const int buf = c & 1;
#pragma unroll
        for (int s = 0; s < kMultiSteps; ++s) {
#pragma unroll
            for (int j = 0; j < W; ++j) {
                const d2 p = tile[buf][j][s * 64 + lane];
#pragma unroll
                for (int i = 0; i < R; ++i) {
                    acc[i * W + j] = fma(a[s][i].x, p.x, acc[i * W + j]);
                    acc[i * W + j] = fma(a[s][i].y, p.y, acc[i * W + j]);
                }
            }
        }
        if (c + 1 < nchunks) stage_store(c + 1, buf ^ 1);
        __syncthreads();
    }

    // every lane group of 64 / NV lanes holds the total of one (row, column) pair
    const int vi = wave_sum_rows<NV>(acc, lane);
    const int i = vi / W, j = vi % W;
    const long row = row_w + i;
    double pv = 0.0;
    if ((lane & (64 / NV - 1)) == 0) {
        if (row < n && s_live[j]) {
            const double y = acc[0];
            Y[(long)j * lda + row] = y;
            const long off = (long)j * lda + row;
            const double pr = FUSED ? fma(s_beta[j], v[off], r[off]) : v[off];   // the p_j[row] this launch staged
            pv = pr * y;                                                          // cg.cc:105
        }
        red[w][vi] = pv;
    }
    __syncthreads();
    if (tid < W && s_live[tid]) {
        double s = 0.0;
        for (int ww = 0; ww < kMultiWaves; ++ww)
#pragma unroll
            for (int ii = 0; ii < R; ++ii) s += red[ww][ii * W + tid];
        partials[(long)tid * gridDim.x + blockIdx.x] = s;
    }
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
        (void)multi_head(ms, rrp, g3, j, k, tol, true, &beta);
    }
}

// Per column j (one workgroup each): ||Y_j - b_j||^2, ||b_j||^2, ||x_j||^2 (cg.cc:146-151) in a fixed order.
__global__ __launch_bounds__(1024) void k_multi_norms(int n, long lda, const double *__restrict__ Y, const double *__restrict__ b,
                                                      const double *__restrict__ x, MultiScalars *ms)
{
    __shared__ double lds[3][16];
    const int j = blockIdx.x;
    double e = 0.0, bb = 0.0, xx = 0.0;
    for (long i = threadIdx.x; i < n; i += 1024) {
        const long off = (long)j * lda + i;
        const double bi = b[off], xi = x[off], d = Y[off] - bi;
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
        ms->norms[j][threadIdx.x] = s;
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
    switch (multi_width(g.nrhs)) {
    case 1: return launch_width<1>(g, fused, s, e0, e1);
    case 2: return launch_width<2>(g, fused, s, e0, e1);
    case 4: return launch_width<4>(g, fused, s, e0, e1);
    case 8: return launch_width<8>(g, fused, s, e0, e1);
    default: return launch_width<16>(g, fused, s, e0, e1);
    }
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

hipError_t launch_multi_norms(int n, long lda, int nrhs, const double *Y, const double *b, const double *x, MultiScalars *ms,
                              hipStream_t s)
{
    hipLaunchKernelGGL(k_multi_norms, dim3(nrhs), dim3(1024), 0, s, n, lda, Y, b, x, ms);
    return hipGetLastError();
}

}  // namespace cgx
