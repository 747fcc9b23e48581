// cgx_lowrank_cols.h -- the pivoted-Cholesky preconditioner applied to a block of up to kMaxRhs columns, device code: THE body of
// the two-launch K3m of cgx_multi_pc.hip (preconditioned CG) and of cgx_lanczos_pc.hip (preconditioned
// Lanczos, section 18).  z_j = (r_j - L C^-1 L^T r_j) / delta in two launches of ONE workgroup per 256-row tile that serve every
// live column, so that the tile of L (256 x rank doubles) is read from memory once per launch, not once per column:
//   lr_tile_partials   ends the first launch (k_multi_lr_update, k_lpc_lr_step: their heads and row updates differ and stay in
//                      their files): with the tile of every r_j in LDS, the tile's partials of t_j = L^T r_j
//   lr_apply_cols      is the second launch (k_multi_lr_apply, k_lpc_lr_apply: wrappers that say which columns are live): t_j folded
//                      over the tiles, u_j = C^-1 t_j, z_j, the r.z partial
// Per (row, column) the chains are k_lr_update's and k_lr_apply's (cgx_lowrank.hip, which folds its tiles with lr_fold_tiles too):
// z_j for a given r_j has the bits the single path gives it, and no sum depends on the column's position among the others.
#pragma once

#include "cgx_device.h"

namespace cgx {

constexpr int kPcGroups = 4;                               // groups of 256 threads per workgroup of the first launch
constexpr int kPcThreads = 256 * kPcGroups;

// the four waves' totals in block_sum<4>'s order
__device__ __forceinline__ double fold4(const double (*red)[kMaxRhs], int j)
{
    return ((red[0][j] + red[1][j]) + red[2][j]) + red[3][j];
}

// the apply launch's shape for a kernel width: NG thread groups of 256, each with CW = W / NG columns (j = q, q + NG, ...)
template <int W>
struct LrColsShape {
    static constexpr int NG = W < kPcGroups ? W : kPcGroups;
    static constexpr int CW = W / NG;
};

// The sum of the G tile partials tp[0], tp[kLrLd], ... in ascending tile order: one chain from +0.0, full trips of 16 loads in
// flight, then the tail one by one.  tp walks, so that a trip's loads are 16 constant offsets from one base and all of them are
// issued ahead of the first add.
__device__ __forceinline__ double lr_fold_tiles(const double *tp, int G)
{
    double s = 0.0;
    int g = 0;
    for (; g + 16 <= G; g += 16, tp += 16 * kLrLd) {
        double a[16];
#pragma unroll
        for (int t = 0; t < 16; ++t) a[t] = tp[t * kLrLd];
#pragma unroll
        for (int t = 0; t < 16; ++t) s += a[t];
    }
    for (; g < G; ++g, tp += kLrLd) s += *tp;
    return s;
}

// acc[c] = sum_u col[u * stride] * vec[j0 + dj c][u] for CW columns at once: per column lr_chain<16>'s chain (cgx_lowrank.hip) --
// one fma chain from +0.0 in ascending u, full trips of 16, the columns past count clamped to the last one and met by vec's
// zeros -- with every trip's 16 values loaded once for all of them.
template <int CW>
__device__ __forceinline__ void lr_chain_cols(const double *__restrict__ col, long stride, const double (*vec)[kLrMaxRank], int j0,
                                              int dj, int count, double (&acc)[CW])
{
#pragma unroll
    for (int c = 0; c < CW; ++c) acc[c] = 0.0;
    for (int u = 0; u < count; u += 16) {
        double w[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) w[q] = col[(long)(u + q < count ? u + q : count - 1) * stride];
#pragma unroll
        for (int q = 0; q < 16; ++q)
#pragma unroll
            for (int c = 0; c < CW; ++c) acc[c] = fma(w[q], vec[j0 + dj * c][u + q], acc[c]);
    }
}

// The end of the first launch (kPcThreads threads, workgroup b = rows [base, base + 256) of every column): with the tile of every
// live r_j in rl (rows past n exactly 0), tpart[j][b][u] = sum over the tile of L[i][u] r_j[i] -- k_lr_update's sums (four rows per
// lane in ascending order, one 8-row wave fold per group of eight columns of L): the groups of eight columns go over the 16
// waves, and the 32 values of L a lane loads serve all columns.
__device__ __forceinline__ void lr_tile_partials(const double (*rl)[256], const int *live, int ncols, const double *__restrict__ L,
                                                 long lda, int rank, int n, int base, double *__restrict__ tpart)
{
    const int lane = (int)threadIdx.x & 63, w = (int)threadIdx.x >> 6;
    const int last = n - 1 - base;                         // >= 0: the grid has no workgroup past n
    int ro[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) ro[q] = (lane + 64 * q) <= last ? lane + 64 * q : last;   // clamped: r is 0 there
    for (int g = w; 8 * g < rank; g += kPcThreads / 64) {
        double lv[8][4];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const int u = 8 * g + c;
            const double *col = L + (long)(u < rank ? u : rank - 1) * lda + base;
#pragma unroll
            for (int q = 0; q < 4; ++q) lv[c][q] = col[ro[q]];
        }
        for (int j = 0; j < ncols; ++j) {
            if (!live[j]) continue;                        // uniform
            double rq[4], v[8];
#pragma unroll
            for (int q = 0; q < 4; ++q) rq[q] = rl[j][lane + 64 * q];
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                double s = 0.0;
#pragma unroll
                for (int q = 0; q < 4; ++q) s = fma(lv[c][q], rq[q], s);
                v[c] = 8 * g + c < rank ? s : 0.0;
            }
            const int row = wave_sum_rows<8>(v, lane);
            if ((lane & 7) == 0 && 8 * g + row < rank) tpart[((long)j * gridDim.x + blockIdx.x) * kLrLd + 8 * g + row] = v[0];
        }
    }
}

// The second launch, 256 * NG threads: workgroup b = the same tile of every live column; thread group q (one thread per row) takes
// the columns j = q, q + NG, ...  t_j = the G tile partials in ascending order (k_lr_apply's fold), u_j = C^-1 t_j in place of
// t_j, z_j = (r_j - L u_j) / delta for the tile's rows, the r.z partial; C^-1's and L's entries are loaded once per 16-column
// trip and used for all CW columns.  live(j): whether column j < ncols runs (the one thing the two callers differ in); a column
// that does not has nothing written.
template <int W, class Live>
__device__ __forceinline__ void lr_apply_cols(Live live, int n, long lda, int ncols, const double *__restrict__ r,
                                              double *__restrict__ z, const double *__restrict__ L, int rank,
                                              const double *__restrict__ Cinv, const LrHead *head,
                                              const double *__restrict__ tpart, double *__restrict__ rzp)
{
    constexpr int NG = LrColsShape<W>::NG, CW = LrColsShape<W>::CW;
    __shared__ double tu[W][kLrMaxRank];
    __shared__ double red[4][kMaxRhs];
    __shared__ int s_live[W];
    const int tid = (int)threadIdx.x, lane = tid & 63;
    const int lt = tid & 255, q = tid >> 8, wl = (tid >> 6) & 3;   // row of the tile, thread group, wave of the group
    const int G = (int)gridDim.x;
    if (tid < W) s_live[tid] = (tid < ncols && live(tid)) ? 1 : 0;
    __syncthreads();
    int any = 0;
#pragma unroll
    for (int j = 0; j < W; ++j) any |= s_live[j];
    if (!any) return;                                      // every column is frozen (uniform)
    const double delta = head->delta;
    const int i = (int)blockIdx.x * 256 + lt;
    const bool in = i < n;
    const long ic = in ? i : n - 1;
    double r_i[CW];
#pragma unroll
    for (int c = 0; c < CW; ++c) {
        const int j = q + NG * c;
        r_i[c] = r[(long)(j < ncols ? j : ncols - 1) * lda + ic];
    }
    for (int c = 0; c < CW; ++c) {
        const int j = q + NG * c;
        double s = 0.0;
        if (s_live[j]) s = lr_fold_tiles(tpart + (long)j * G * kLrLd + (lt < rank ? lt : 0), G);   // uniform over the group
        tu[j][lt] = (lt < rank && s_live[j]) ? s : 0.0;    // zeros behind the rank: the chain's last trip
    }
    __syncthreads();
    double acc[CW];
    // C^-1 is symmetric bit for bit: row lt read as column lt, coalesced
    lr_chain_cols<CW>(Cinv + (lt < rank ? lt : 0), kLrLd, tu, q, NG, rank, acc);
    __syncthreads();
#pragma unroll
    for (int c = 0; c < CW; ++c) tu[q + NG * c][lt] = lt < rank ? acc[c] : 0.0;
    __syncthreads();
    lr_chain_cols<CW>(L + ic, lda, tu, q, NG, rank, acc);
#pragma unroll
    for (int c = 0; c < CW; ++c) {
        const int j = q + NG * c;
        double rz = 0.0;
        if (s_live[j]) {                                   // uniform over the group
            if (in) {
                const double zv = (r_i[c] - acc[c]) / delta;
                z[(long)j * lda + i] = zv;
                rz = r_i[c] * zv;
            }
            rz = wave_sum(rz);
            if (lane == 0) red[wl][j] = rz;
        }
    }
    __syncthreads();
    if (tid < W && s_live[tid]) rzp[(long)tid * G + blockIdx.x] = fold4(red, tid);
}

}  // namespace cgx
