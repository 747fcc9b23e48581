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
//               the single path gives it.  The end of the update (lr_tile_partials) and the whole apply (lr_apply_cols) are ONE
//               body in cgx_lowrank_cols.h, which cgx_lanczos_pc.hip's pair runs too; here are the update's head -- alpha_j and
//               the rows of CG -- and what makes a column live: MultiScalars::done.
//
// A frozen column has nothing written (x, r, z, p, scalars, partials); columns nrhs .. W-1 are masked by nrhs.  No floating-point
// atomics; every sum has a fixed order that does not depend on the column's position among the others.
#include "cgx_kernels.h"
#include "cgx_lowrank_cols.h"

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

// K3m, pivoted Cholesky, the update launch: workgroup b = rows [256 b, 256 b + 256) of EVERY live column, 1024 threads.  Thread
// group q (256 threads, one per row) takes the columns j = q, q + 4, ...: p.Ap from K1m's g1 partials in K3's order, alpha_j,
// x_j += alpha_j p_j, r_j -= alpha_j Y_j, the r.r partial (per column the sums of k_multi_update: a wave's 64 rows, then the
// group's four waves in order).  Then, with the tile of every r_j in LDS, the tile's partials of t_j = L^T r_j (lr_tile_partials).
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
    lr_tile_partials(rl, s_live, nrhs, L, lda, rank, n, base, tpart);
}

// K3m, pivoted Cholesky, the apply launch (lr_apply_cols): z_j = M^-1 r_j and the r.z partials of the columns that have not taken
// the break.  ms == nullptr: no frozen columns (set-up, probe).
template <int W>
__global__ __launch_bounds__(256 * LrColsShape<W>::NG) void k_multi_lr_apply(int n, long lda, int nrhs, const double *__restrict__ r,
                                                                             double *__restrict__ z, const double *__restrict__ L,
                                                                             int rank, const double *__restrict__ Cinv,
                                                                             const LrHead *head, const double *__restrict__ tpart,
                                                                             const MultiScalars *ms, double *__restrict__ rzp)
{
    lr_apply_cols<W>([ms](int j) { return !(ms && ms->done[j]); }, n, lda, nrhs, r, z, L, rank, Cinv, head, tpart, rzp);
}

template <int W>
hipError_t launch_gemv_width(const MultiArgs &g, const MultiPcArgs &pc, hipStream_t s, hipEvent_t e0, hipEvent_t e1)
{
    hipExtLaunchKernelGGL((k_multi_gemv_pc<W>), dim3(multi_gemv_grid(g.n, W)), dim3(kMultiThreads), 0, s, e0, e1, 0, g.A, g.lda, g.n,
                          g.nrhs, g.v, g.p_new, g.r, pc.rzp, g.rrp, multi_update_grid(g.n), g.Y, g.partials, g.ms, pc.mp, g.k, g.tol);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_multi_gemv_pc(const MultiArgs &g, const MultiPcArgs &pc, hipStream_t s, hipEvent_t e0, hipEvent_t e1)
{
    if (g.nrhs < 1 || g.nrhs > kMaxRhs || g.n < 1) return hipErrorInvalidValue;
    return for_multi_width(g.nrhs, [&](auto w) { return launch_gemv_width<decltype(w)::value>(g, pc, s, e0, e1); });
}

hipError_t launch_multi_update_pc(int n, long lda, int nrhs, const double *p, const double *Y, const double *partials, int g1, double *x,
                                  double *r, double *rrp, MultiScalars *ms, int parity, const MultiPcArgs &pc, bool init, hipStream_t s)
{
    if (nrhs < 1 || nrhs > kMaxRhs || n < 1 || !pc_factor_ok(n, pc.M)) return hipErrorInvalidValue;
    const PcFactor &M = pc.M;
    const int g3 = multi_update_grid(n);
    if (M.dinv) {
        if (init)
            hipLaunchKernelGGL((k_multi_update_jac<true>), dim3(g3, nrhs), dim3(256), 0, s, n, lda, p, Y, partials, g1, x, r, pc.Z, M.dinv,
                               pc.rzp, rrp, ms, parity);
        else
            hipLaunchKernelGGL((k_multi_update_jac<false>), dim3(g3, nrhs), dim3(256), 0, s, n, lda, p, Y, partials, g1, x, r, pc.Z, M.dinv,
                               pc.rzp, rrp, ms, parity);
        return hipGetLastError();
    }
    if (init)
        hipLaunchKernelGGL((k_multi_lr_update<true>), dim3(g3), dim3(kPcThreads), 0, s, n, lda, nrhs, p, Y, partials, g1, x, r, rrp, ms, parity,
                           M.L, M.rank, M.tpart);
    else
        hipLaunchKernelGGL((k_multi_lr_update<false>), dim3(g3), dim3(kPcThreads), 0, s, n, lda, nrhs, p, Y, partials, g1, x, r, rrp, ms, parity,
                           M.L, M.rank, M.tpart);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const MultiScalars *frozen = init ? nullptr : ms;
    return for_multi_width(nrhs, [&](auto w) {
        constexpr int W = decltype(w)::value;
        hipLaunchKernelGGL((k_multi_lr_apply<W>), dim3(g3), dim3(256 * LrColsShape<W>::NG), 0, s, n, lda, nrhs, r, pc.Z, M.L, M.rank, M.Cinv,
                           M.head, M.tpart, frozen, pc.rzp);
        return hipGetLastError();
    });
}

hipError_t launch_multi_close_pc(MultiScalars *ms, const MultiPcArgs &pc, const double *rrp, int n, int nrhs, int k, double tol,
                                 hipStream_t s)
{
    hipLaunchKernelGGL(k_multi_close_pc, dim3(1), dim3(kMultiThreads), 0, s, ms, pc.mp, pc.rzp, rrp, multi_update_grid(n), nrhs, k, tol);
    return hipGetLastError();
}

}  // namespace cgx
