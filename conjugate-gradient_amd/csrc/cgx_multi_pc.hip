// cgx_multi_pc.hip -- several right-hand sides with a preconditioner on one GPU (cgx_solve_multi_pc):
// k independent copies of the recurrence of section 11, one per column of the k-wide blocks of cgx_multi.hip plus Z = M^-1 R.
//
//   K1m fused   the body of cgx_multi.hip's (cgx_multi_gemv.inc, PRE = true): per column the head folds the r.z and the r.r
//               partials, rho_j = r_j.z_j gives beta_j, sqrt(r_j.r_j) < tol the break; p_j = z_j + beta_j p_j; Y = A P
//   K3m Jacobi  k_multi_update plus z = dinv r_new (pc_update_row: the single path's row) and the two partials per (tile, column)
//   K3m pivoted Cholesky, two launches of ONE workgroup per 256-row tile that serve every live column, so that the tile of L
//               (256 x rank doubles) is read from memory once per launch, not once per column; a workgroup is up to four groups of
//               256 threads (one per row) that share the columns among themselves:
//               update   per column alpha_j, x_j, r_j, the r.r partial and, with r_j's tile in LDS, the tile's partials of
//                        t_j = L^T r_j -- every group of eight columns of L is loaded into registers once and used for all columns
//               apply    t_j folded over the tiles in ascending order, u_j = C^-1 t_j, z_j = (r_j - L u_j) / delta, r.z partial;
//                        C^-1's and L's entries are loaded once per 16-column trip and used for all W columns
//               Per (row, column) the chains are k_lr_update's and k_lr_apply's (cgx_lowrank.hip): z_j for a given r_j has the bits
//               the single path gives it.
//
// A frozen column has nothing written (x, r, z, p, scalars, partials); columns nrhs .. W-1 are masked by nrhs.  No floating-point
// atomics; every sum has a fixed order that does not depend on the column's position among the others.
#include "cgx_kernels.h"
#include "cgx_device.h"

#include <hip/hip_ext.h>

namespace cgx {

namespace {

template <int W>
__global__ __launch_bounds__(kMultiThreads, 2) void k_multi_gemv_pc(const double *__restrict__ A, long lda, int n, int nrhs,
                                                                    const double *__restrict__ v, double *__restrict__ p_new,
                                                                    const double *__restrict__ r, const double *__restrict__ rzp,
                                                                    const double *__restrict__ rrp, int g3, double *__restrict__ Y,
                                                                    double *__restrict__ partials, MultiScalars *ms,
                                                                    MultiPcScalars *mp, int k, double tol)
{
    constexpr bool FUSED = true;   // v is p_old, r is z = M^-1 r
    constexpr bool PRE = true;
#include "cgx_multi_gemv.inc"
}

// The loop ran out after k iterations: the head of iteration k for every column (what the next K1m would have done).
__global__ __launch_bounds__(kMultiThreads) void k_multi_close_pc(MultiScalars *ms, MultiPcScalars *mp, const double *__restrict__ rzp,
                                                                  const double *__restrict__ rrp, int g3, int nrhs, int k, double tol)
{
    const int w = threadIdx.x >> 6;
    for (int j = w; j < nrhs; j += kMultiWaves) {
        double beta;
        (void)multi_head<true>(ms, mp, rzp, rrp, g3, j, k, tol, true, &beta);
    }
}

// the four waves' totals in block_sum<4>'s order
__device__ __forceinline__ double fold4(const double (*red)[kMaxRhs], int j)
{
    return ((red[0][j] + red[1][j]) + red[2][j]) + red[3][j];
}

// K3m, Jacobi: workgroup (b, j) = rows [256 b, 256 b + 256) of column j, as k_multi_update; rho_j = ms->rs[j][parity].
// INIT: r is taken as it is (z0 and both partial sets behind k_multi_init).
template <bool INIT>
__global__ __launch_bounds__(256) void k_multi_update_jac(int n, long lda, const double *__restrict__ p, const double *__restrict__ Y,
                                                          const double *__restrict__ partials, int g1, double *__restrict__ x,
                                                          double *__restrict__ r, double *__restrict__ z,
                                                          const double *__restrict__ dinv, double *__restrict__ rzp,
                                                          double *__restrict__ rrp, MultiScalars *ms, int parity)
{
    __shared__ double lds[4];
    const int j = blockIdx.y;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const long off = (long)j * lda + i;
    const bool in = i < n;
    const double dinv_i = in ? dinv[i] : 0.0;
    PcRow row{0.0, 0.0, 0.0, 0.0};
    if constexpr (INIT) {
        if (in) row = pc_row(r[off], dinv_i);
    } else {
        const int done = ms->done[j];
        const double rho = ms->rs[j][parity];
        double ap_i = 0.0, r_i = 0.0, p_i = 0.0, x_i = 0.0;
        if (in) { ap_i = Y[off]; r_i = r[off]; p_i = p[off]; x_i = x[off]; }
        const double cs = fold_pap(partials + (long)j * g1, 1, 0, g1);
        if (done) return;                                  // frozen column (uniform over the workgroup)
        const double conj = block_sum<4>(cs, lds);
        const double alpha = safeguarded_alpha(rho, conj);
        if (in) {
            row = pc_update_row(alpha, ap_i, r_i, dinv_i);
            r[off] = row.r;
            x[off] = fma(alpha, p_i, x_i);
        }
    }
    if (in) z[off] = row.z;
    const double rz = block_sum<4>(row.rz, lds);
    const double rr = block_sum<4>(row.rr, lds);
    if (threadIdx.x == 0) {
        rzp[(long)j * gridDim.x + blockIdx.x] = rz;
        rrp[(long)j * gridDim.x + blockIdx.x] = rr;
    }
}

constexpr int kPcGroups = 4;                               // groups of 256 threads per workgroup of the update launch
constexpr int kPcThreads = 256 * kPcGroups;

// K3m, pivoted Cholesky, the update launch: workgroup b = rows [256 b, 256 b + 256) of EVERY live column, 1024 threads.  Thread
// group q (256 threads, one per row) takes the columns j = q, q + 4, ...: p.Ap from K1m's g1 partials in K3's order, alpha_j,
// x_j += alpha_j p_j, r_j -= alpha_j Y_j, the r.r partial (per column the sums of k_multi_update: a wave's 64 rows, then the
// group's four waves in order).  Then, with the tile of every r_j in LDS, tpart[j][b][u] = sum over the tile of L[i][u] r_j[i] --
// k_lr_update's sums (four rows per lane in ascending order, one 8-row wave fold per group of eight columns of L): the groups
// of eight columns go over the 16 waves, and the 32 values of L a lane loads serve all columns.
template <bool INIT>
__global__ __launch_bounds__(kPcThreads) void k_multi_lr_update(int n, long lda, int nrhs, const double *__restrict__ p,
                                                                const double *__restrict__ Y, const double *__restrict__ partials,
                                                                int g1, double *__restrict__ x, double *__restrict__ r,
                                                                double *__restrict__ rrp, const MultiScalars *ms, int parity,
                                                                const double *__restrict__ L, int rank, double *__restrict__ tpart)
{
    __shared__ double rl[kMaxRhs][256];
    __shared__ double red[4][kMaxRhs];
    __shared__ double red2[4][kMaxRhs];
    __shared__ double s_alpha[kMaxRhs];
    __shared__ int s_live[kMaxRhs];
    const int tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int lt = tid & 255, q4 = tid >> 8, wl = w & 3;   // row of the tile, thread group, wave of the group
    const int base = (int)blockIdx.x * 256;
    const int i = base + lt;
    const bool in = i < n;
    const long ic = in ? i : n - 1;                        // clamped: every load is unconditional
    if (tid < kMaxRhs) {
        bool live = tid < nrhs;
        if constexpr (!INIT) live = live && !ms->done[tid];
        s_live[tid] = live ? 1 : 0;
    }
    __syncthreads();
    if constexpr (!INIT) {
        for (int j = q4; j < nrhs; j += kPcGroups) {
            if (!s_live[j]) continue;                      // frozen column (uniform over the group)
            const double cs = wave_sum(fold_pap(partials + (long)j * g1, 1, 0, g1, lt));
            if (lane == 0) red[wl][j] = cs;
        }
        __syncthreads();
        if (tid < nrhs && s_live[tid]) s_alpha[tid] = safeguarded_alpha(ms->rs[tid][parity], fold4(red, tid));   // rho / p.Ap
        __syncthreads();
    }
    {
        constexpr int CG = kMaxRhs / kPcGroups;            // columns per group at most: their loads are in flight together
        double ap_i[CG], r_i[CG], p_i[CG], x_i[CG];
#pragma unroll
        for (int u = 0; u < CG; ++u) {
            const int j = q4 + kPcGroups * u, jc = j < nrhs ? j : nrhs - 1;
            const long off = (long)jc * lda + ic;
            r_i[u] = r[off];
            if constexpr (!INIT) { ap_i[u] = Y[off]; p_i[u] = p[off]; x_i[u] = x[off]; }
        }
#pragma unroll
        for (int u = 0; u < CG; ++u) {
            const int j = q4 + kPcGroups * u;
            if (j >= nrhs || !s_live[j]) continue;         // uniform over the group
            const long off = (long)j * lda + i;
            double rn = in ? r_i[u] : 0.0;
            if constexpr (!INIT) {
                if (in) {
                    const double alpha = s_alpha[j];
                    rn = fma(-alpha, ap_i[u], r_i[u]);
                    r[off] = rn;
                    x[off] = fma(alpha, p_i[u], x_i[u]);
                }
            }
            rl[j][lt] = rn;                                // rows past n: exactly 0
            const double rr = wave_sum(rn * rn);
            if (lane == 0) red2[wl][j] = rr;
        }
    }
    __syncthreads();                                       // publishes rl and red2
    if (tid < nrhs && s_live[tid]) rrp[(long)tid * gridDim.x + blockIdx.x] = fold4(red2, tid);
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
        for (int j = 0; j < nrhs; ++j) {
            if (!s_live[j]) continue;                      // uniform
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

// the apply launch's shape for a kernel width: NG thread groups of 256, each with CW = W / NG columns (j = q, q + NG, ...)
template <int W>
struct ApplyShape {
    static constexpr int NG = W < kPcGroups ? W : kPcGroups;
    static constexpr int CW = W / NG;
};

// K3m, pivoted Cholesky, the apply launch: workgroup b = the same tile of every live column; thread group q (one thread per row)
// takes the columns j = q, q + NG, ...  t_j = the G tile partials in ascending order (k_lr_apply's fold), u_j = C^-1 t_j in place
// of t_j, z_j = (r_j - L u_j) / delta for the tile's rows, the r.z partial.  ms == nullptr: no frozen columns (set-up, probe).
template <int W>
__global__ __launch_bounds__(256 * ApplyShape<W>::NG) void k_multi_lr_apply(int n, long lda, int nrhs, const double *__restrict__ r,
                                                                            double *__restrict__ z, const double *__restrict__ L,
                                                                            int rank, const double *__restrict__ Cinv,
                                                                            const LrHead *head, const double *__restrict__ tpart,
                                                                            const MultiScalars *ms, double *__restrict__ rzp)
{
    constexpr int NG = ApplyShape<W>::NG, CW = ApplyShape<W>::CW;
    __shared__ double tu[W][kLrMaxRank];
    __shared__ double red[4][kMaxRhs];
    __shared__ int s_live[W];
    const int tid = (int)threadIdx.x, lane = tid & 63;
    const int lt = tid & 255, q = tid >> 8, wl = (tid >> 6) & 3;   // row of the tile, thread group, wave of the group
    const int G = (int)gridDim.x;
    if (tid < W) s_live[tid] = (tid < nrhs && !(ms && ms->done[tid])) ? 1 : 0;
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
        r_i[c] = r[(long)(j < nrhs ? j : nrhs - 1) * lda + ic];
    }
    for (int c = 0; c < CW; ++c) {
        const int j = q + NG * c;
        double s = 0.0;
        if (s_live[j]) {                                   // uniform over the group
            const double *tp = tpart + (long)j * G * kLrLd + (lt < rank ? lt : 0);
            int g = 0;
            for (; g + 16 <= G; g += 16) {
                double a[16];
#pragma unroll
                for (int t = 0; t < 16; ++t) a[t] = tp[(long)(g + t) * kLrLd];
#pragma unroll
                for (int t = 0; t < 16; ++t) s += a[t];
            }
            for (; g < G; ++g) s += tp[(long)g * kLrLd];
        }
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

template <int W>
hipError_t launch_gemv_width(const MultiArgs &g, const MultiPcArgs &pc, hipStream_t s, hipEvent_t e0, hipEvent_t e1)
{
    hipExtLaunchKernelGGL((k_multi_gemv_pc<W>), dim3(multi_gemv_grid(g.n, W)), dim3(kMultiThreads), 0, s, e0, e1, 0, g.A, g.lda, g.n,
                          g.nrhs, g.v, g.p_new, g.r, pc.rzp, g.rrp, multi_update_grid(g.n), g.Y, g.partials, g.ms, pc.mp, g.k, g.tol);
    return hipGetLastError();
}

template <int W>
hipError_t launch_apply_width(int n, long lda, int nrhs, const double *r, const MultiPcArgs &pc, const MultiScalars *ms, hipStream_t s)
{
    hipLaunchKernelGGL((k_multi_lr_apply<W>), dim3(lr_grid(n)), dim3(256 * ApplyShape<W>::NG), 0, s, n, lda, nrhs, r, pc.Z, pc.L, pc.rank, pc.Cinv, pc.head,
                       pc.tpart, ms, pc.rzp);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_multi_gemv_pc(const MultiArgs &g, const MultiPcArgs &pc, hipStream_t s, hipEvent_t e0, hipEvent_t e1)
{
    if (g.nrhs < 1 || g.nrhs > kMaxRhs || g.n < 1) return hipErrorInvalidValue;
    switch (multi_width(g.nrhs)) {
    case 1: return launch_gemv_width<1>(g, pc, s, e0, e1);
    case 2: return launch_gemv_width<2>(g, pc, s, e0, e1);
    case 4: return launch_gemv_width<4>(g, pc, s, e0, e1);
    case 8: return launch_gemv_width<8>(g, pc, s, e0, e1);
    default: return launch_gemv_width<16>(g, pc, s, e0, e1);
    }
}

hipError_t launch_multi_update_pc(int n, long lda, int nrhs, const double *p, const double *Y, const double *partials, int g1, double *x,
                                  double *r, double *rrp, MultiScalars *ms, int parity, const MultiPcArgs &pc, bool init, hipStream_t s)
{
    if (nrhs < 1 || nrhs > kMaxRhs || n < 1) return hipErrorInvalidValue;
    const int g3 = multi_update_grid(n);
    if (pc.dinv) {
        if (init)
            hipLaunchKernelGGL((k_multi_update_jac<true>), dim3(g3, nrhs), dim3(256), 0, s, n, lda, p, Y, partials, g1, x, r, pc.Z, pc.dinv,
                               pc.rzp, rrp, ms, parity);
        else
            hipLaunchKernelGGL((k_multi_update_jac<false>), dim3(g3, nrhs), dim3(256), 0, s, n, lda, p, Y, partials, g1, x, r, pc.Z, pc.dinv,
                               pc.rzp, rrp, ms, parity);
        return hipGetLastError();
    }
    if (pc.rank < 1 || pc.rank > kLrMaxRank || g3 != lr_grid(n) || g3 > kMaxVectorGrid) return hipErrorInvalidValue;
    if (init)
        hipLaunchKernelGGL((k_multi_lr_update<true>), dim3(g3), dim3(kPcThreads), 0, s, n, lda, nrhs, p, Y, partials, g1, x, r, rrp, ms, parity,
                           pc.L, pc.rank, pc.tpart);
    else
        hipLaunchKernelGGL((k_multi_lr_update<false>), dim3(g3), dim3(kPcThreads), 0, s, n, lda, nrhs, p, Y, partials, g1, x, r, rrp, ms, parity,
                           pc.L, pc.rank, pc.tpart);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const MultiScalars *frozen = init ? nullptr : ms;
    switch (multi_width(nrhs)) {
    case 1: return launch_apply_width<1>(n, lda, nrhs, r, pc, frozen, s);
    case 2: return launch_apply_width<2>(n, lda, nrhs, r, pc, frozen, s);
    case 4: return launch_apply_width<4>(n, lda, nrhs, r, pc, frozen, s);
    case 8: return launch_apply_width<8>(n, lda, nrhs, r, pc, frozen, s);
    default: return launch_apply_width<16>(n, lda, nrhs, r, pc, frozen, s);
    }
}

hipError_t launch_multi_close_pc(MultiScalars *ms, const MultiPcArgs &pc, const double *rrp, int n, int nrhs, int k, double tol,
                                 hipStream_t s)
{
    hipLaunchKernelGGL(k_multi_close_pc, dim3(1), dim3(kMultiThreads), 0, s, ms, pc.mp, pc.rzp, rrp, multi_update_grid(n), nrhs, k, tol);
    return hipGetLastError();
}

}  // namespace cgx
