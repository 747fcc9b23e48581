// cgx_lanczos_pc.hip -- the update kernels of the PRECONDITIONED multi-vector Lanczos recurrence (cgx_lanczos_pc, cgx_trace_slq_pc,
// cgx_slq_probes), beside cgx_lanczos.hip and cgx_multi_pc.hip, which stay as they are.
//
// Per column j of a block of up to kMaxRhs vectors (column-major at pitch lda), with M the context's preconditioner (M = D for
// point Jacobi, M = L L^T + delta I for the pivoted-Cholesky factor):
//
//   w_0 = V0_j, u_0 = M^-1 w_0, eta0^2 = w_0 . u_0, v_-1 = 0, beta_-1 := eta0
//   step t:  v_t = w_t / beta_(t-1);  q_t = u_t / beta_(t-1);  y = A q_t;  alpha_t = q_t . y
//            w_(t+1) = y - alpha_t v_t - beta_(t-1) v_(t-1);  u_(t+1) = M^-1 w_(t+1);  beta_t = sqrt(w_(t+1) . u_(t+1))
//
// The mat-vec is the plain multi-vector K1 (cgx_multi.hip, untouched), run on the NOT YET NORMALISED u_t: it leaves Y = A u_t and
// the partials of u_t . A u_t.  Behind it, step t is
//   Jacobi             ONE launch, workgroup (b, j) = rows [256 b, 256 b + 256) of column j: beta_(t-1) = sqrt of the w.u partials the
//                      previous step left, the breakdown test, alpha_t = (u_t . A u_t) / beta^2, per row v = w / beta, y = Y / beta,
//                      w' = fma(-beta, v_prev, fma(-alpha, v, y)), v over w, w' over v_prev, u' = dinv w', one w'.u' partial
//   pivoted Cholesky   TWO launches of one workgroup per 256-row tile that serve every live column, shaped as cgx_multi_pc.hip's pair
//                      so that the tile of L is read once per launch: the step (scalars and rows as above, and the tile's partials
//                      of t_j = L^T w'_j) and the apply (t_j folded in ascending tile order, u_j = C^-1 t_j, u' = (w' - L u_j) /
//                      delta, the w'.u' partial).  The end of the step (lr_tile_partials) and the whole apply (lr_apply_cols) are
//                      the ONE body of cgx_lowrank_cols.h that cgx_multi_pc.hip's pair runs; here are the step's head and rows,
//                      and what makes a column live: LanczosScalars::m, not MultiScalars::done.
// The host swaps w and v_prev between steps.  The set-up is the same launches in their INIT form (w taken as it is, v_prev = 0)
// plus k_lpc_begin, which folds eta0^2 as every later step folds its partials and resets the column's scalars.
//
// Every workgroup of a column folds the same partials in the same fixed order (fold_pap, wave sums, the four waves in order) and
// so takes the same decision; the workgroup of tile 0 alone writes the column's scalars and histories, with plain stores.  The
// running max |alpha| is a ping-pong pair and "frozen" is a step number, so no workgroup reads a word another workgroup of the
// same launch writes with a different meaning.  A frozen column has nothing written any more.  No floating-point atomics; no sum
// depends on the column's position in the block; every offset is 64-bit.
#include "cgx_kernels.h"
#include "cgx_lowrank_cols.h"

namespace cgx {

namespace {

constexpr double kLanczosBreak = 0x1.0p-36;   // beta_t <= 2^-36 max |alpha|: an invariant subspace (DESIGN.md sections 17, 18)
constexpr double kDblMax = 1.7976931348623157e308;

// What step t decides for a column from ww = w_t . u_t, wAw = u_t . A u_t and the running max |alpha|; the writer stores it.
struct StepHead {
    double alpha, beta;
    bool run;
};
__device__ __forceinline__ StepHead step_head(double ww, double wAw, double amax, int j, int t, bool writer, LanczosScalars *ls,
                                              double *__restrict__ ha, double *__restrict__ hb)
{
    StepHead h;
    h.beta = ww > 0.0 ? sqrt(ww) : 0.0;                    // beta_(t-1); t = 0: eta0 (checked by k_lpc_begin)
    h.alpha = 0.0;
    const long at = (long)j * kMaxLanczosSteps + t;
    if (writer && t > 0) hb[at - 1] = h.beta;
    h.run = ww > 0.0 && !(h.beta <= kLanczosBreak * amax);
    if (!h.run) {                                          // breakdown: the column is frozen with m = t
        if (writer) ls->m[j] = t;
        return h;
    }
    h.alpha = wAw / ww;
    if (writer) {
        ha[at] = h.alpha;
        const double aa = fabs(h.alpha);
        ls->amax[j][(t + 1) & 1] = aa > amax ? aa : amax;
    }
    return h;
}

// Behind the set-up launches, one workgroup per column: eta0^2 from the w.u partials in the steps' own order, the scalars reset; a
// column whose eta0^2 is 0, negative or not finite is marked bad and never runs.
__global__ __launch_bounds__(256) void k_lpc_begin(const double *__restrict__ wu, int g3, LanczosScalars *ls)
{
    __shared__ double lds[4];
    const int j = blockIdx.x;
    const double tot = block_sum<4>(fold_pap(wu + (long)j * g3, 1, 0, g3), lds);
    if (threadIdx.x == 0) {
        const bool ok = tot > 0.0 && tot <= kDblMax;       // false for 0, negative, inf and NaN
        ls->amax[j][0] = 0.0;
        ls->amax[j][1] = 0.0;
        ls->z2[j] = tot;
        ls->m[j] = ok ? kLanczosLive : -1;
        ls->bad[j] = ok ? 0 : 1;
    }
}

// Jacobi.  Workgroup (b, j) = rows [256 b, 256 b + 256) of column j.  INIT: u = dinv w, v_prev = 0, the w.u partial.
template <bool INIT>
__global__ __launch_bounds__(256) void k_lpc_jac_step(int n, long lda, double *__restrict__ w, double *__restrict__ vprev,
                                                      double *__restrict__ u, const double *__restrict__ Y,
                                                      const double *__restrict__ dinv, const double *__restrict__ k1p, int g1,
                                                      const double *__restrict__ wu_in, double *__restrict__ wu_out,
                                                      LanczosScalars *ls, double *__restrict__ ha, double *__restrict__ hb, int t)
{
    __shared__ double lds[4];
    const int j = blockIdx.y;
    const int g3 = gridDim.x;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const long off = (long)j * lda + i;
    const bool in = i < n;
    const double dinv_i = in ? dinv[i] : 0.0;
    double wn = 0.0;
    if constexpr (INIT) {
        if (in) {
            wn = w[off];
            vprev[off] = 0.0;
        }
    } else {
        const int mj = ls->m[j];
        const double amax = ls->amax[j][t & 1];
        double w_i = 0.0, y_i = 0.0, p_i = 0.0;
        if (in) { w_i = w[off]; y_i = Y[off]; p_i = vprev[off]; }
        const double ws = fold_pap(wu_in + (long)j * g3, 1, 0, g3);
        const double cs = fold_pap(k1p + (long)j * g1, 1, 0, g1);
        if (mj < t) return;                                // frozen in an earlier step (uniform: only step mj writes mj)
        const double ww = block_sum<4>(ws, lds);           // w_t . u_t
        const double wAw = block_sum<4>(cs, lds);          // u_t . A u_t
        const StepHead h = step_head(ww, wAw, amax, j, t, blockIdx.x == 0 && threadIdx.x == 0, ls, ha, hb);
        if (!h.run) return;
        if (in) {
            const double v = w_i / h.beta, y = y_i / h.beta;
            wn = fma(-h.beta, p_i, fma(-h.alpha, v, y));
            w[off] = v;
            vprev[off] = wn;
        }
    }
    const double un = dinv_i * wn;
    if (in) u[off] = un;
    const double nw = block_sum<4>(wn * un, lds);
    if (threadIdx.x == 0) wu_out[(long)j * g3 + blockIdx.x] = nw;
}

// Pivoted Cholesky, the step launch: workgroup b = rows [256 b, 256 b + 256) of EVERY live column, 1024 threads.  Thread group q
// (256 threads, one per row) takes the columns j = q, q + 4, ...: the two folds, the column's decision, the rows.  Then, with the
// tile of every w'_j in LDS, the tile's partials of t_j = L^T w'_j (lr_tile_partials).
// s_live[j] afterwards: the column runs step t (INIT: every column < nvec).
template <bool INIT>
__global__ __launch_bounds__(kPcThreads) void k_lpc_lr_step(int n, long lda, int nvec, double *__restrict__ w,
                                                            double *__restrict__ vprev, const double *__restrict__ Y,
                                                            const double *__restrict__ k1p, int g1, const double *__restrict__ wu_in,
                                                            LanczosScalars *ls, double *__restrict__ ha, double *__restrict__ hb,
                                                            int t, const double *__restrict__ L, int rank,
                                                            double *__restrict__ tpart)
{
    __shared__ double rl[kMaxRhs][256];
    __shared__ double red[4][kMaxRhs];
    __shared__ double red2[4][kMaxRhs];
    __shared__ double s_alpha[kMaxRhs];
    __shared__ double s_beta[kMaxRhs];
    __shared__ int s_live[kMaxRhs];
    const int tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int lt = tid & 255, q4 = tid >> 8, wl = wv & 3;  // row of the tile, thread group, wave of the group
    const int G = (int)gridDim.x;
    const int base = (int)blockIdx.x * 256;
    const int i = base + lt;
    const bool in = i < n;
    const long ic = in ? i : n - 1;                        // clamped: every load is unconditional
    if (tid < kMaxRhs) {
        bool live = tid < nvec;
        if constexpr (!INIT) live = live && ls->m[tid] >= t;   // (only step m writes m: both values read here mean "decides in t")
        s_live[tid] = live ? 1 : 0;
    }
    __syncthreads();
    if constexpr (!INIT) {
        for (int j = q4; j < nvec; j += kPcGroups) {
            if (!s_live[j]) continue;                      // frozen column (uniform over the group)
            const double ws = wave_sum(fold_pap(wu_in + (long)j * G, 1, 0, G, lt));
            const double cs = wave_sum(fold_pap(k1p + (long)j * g1, 1, 0, g1, lt));
            if (lane == 0) { red[wl][j] = ws; red2[wl][j] = cs; }
        }
        __syncthreads();
        if (tid < nvec && s_live[tid]) {
            const StepHead h = step_head(fold4(red, tid), fold4(red2, tid), ls->amax[tid][t & 1], tid, t, blockIdx.x == 0, ls, ha, hb);
            s_alpha[tid] = h.alpha;
            s_beta[tid] = h.beta;
            if (!h.run) s_live[tid] = 0;
        }
        __syncthreads();
    }
    {
        constexpr int CG = kMaxRhs / kPcGroups;            // columns per group at most: their loads are in flight together
        double w_i[CG], y_i[CG], p_i[CG];
#pragma unroll
        for (int c = 0; c < CG; ++c) {
            const int j = q4 + kPcGroups * c, jc = j < nvec ? j : nvec - 1;
            const long off = (long)jc * lda + ic;
            w_i[c] = w[off];
            if constexpr (!INIT) { y_i[c] = Y[off]; p_i[c] = vprev[off]; }
        }
#pragma unroll
        for (int c = 0; c < CG; ++c) {
            const int j = q4 + kPcGroups * c;
            if (j >= nvec || !s_live[j]) continue;         // uniform over the group
            const long off = (long)j * lda + i;
            double wn = in ? w_i[c] : 0.0;
            if constexpr (INIT) {
                if (in) vprev[off] = 0.0;
            } else {
                if (in) {
                    const double beta = s_beta[j], alpha = s_alpha[j];
                    const double v = w_i[c] / beta, y = y_i[c] / beta;
                    wn = fma(-beta, p_i[c], fma(-alpha, v, y));
                    w[off] = v;
                    vprev[off] = wn;
                }
            }
            rl[j][lt] = wn;                                // rows past n: exactly 0
        }
    }
    __syncthreads();                                       // publishes rl
    lr_tile_partials(rl, s_live, nvec, L, lda, rank, n, base, tpart);
}

// Pivoted Cholesky, the apply launch (lr_apply_cols): u'_j = M^-1 w'_j and the w'.u' partials of the columns that ran step t
// (m > t); ls == nullptr: the set-up, every column < nvec.
template <int W>
__global__ __launch_bounds__(256 * LrColsShape<W>::NG) void k_lpc_lr_apply(int n, long lda, int nvec, const double *__restrict__ wn,
                                                                           double *__restrict__ u, const double *__restrict__ L,
                                                                           int rank, const double *__restrict__ Cinv,
                                                                           const LrHead *head, const double *__restrict__ tpart,
                                                                           const LanczosScalars *ls, int t,
                                                                           double *__restrict__ wu_out)
{
    lr_apply_cols<W>([ls, t](int j) { return !(ls && ls->m[j] <= t); }, n, lda, nvec, wn, u, L, rank, Cinv, head, tpart, wu_out);
}

// One workgroup per column: the last beta, and m = steps for a column that ran to the end.
__global__ __launch_bounds__(256) void k_lpc_close(const double *__restrict__ wu, int g3, int steps, LanczosScalars *ls,
                                                   double *__restrict__ hb)
{
    __shared__ double lds[4];
    const int j = blockIdx.x;
    const int mj = ls->m[j];
    const double ws = fold_pap(wu + (long)j * g3, 1, 0, g3);
    if (mj != kLanczosLive) return;
    const double tot = block_sum<4>(ws, lds);
    if (threadIdx.x == 0) {
        hb[(long)j * kMaxLanczosSteps + steps - 1] = tot > 0.0 ? sqrt(tot) : 0.0;
        ls->m[j] = steps;
    }
}

// The probes of cgx_trace_slq_pc / cgx_slq_probes.  Workgroup (b, j) = rows [256 b, 256 b + 256) of probe probe0 + j; s_i = the
// Rademacher sign of (probe, element i) as cgx_trace_slq makes it.  kind 0: z = s (covariance I); kLpcJacobi: z_i = s_i sqrt(A_ii);
// kLpcLowrank: z = L g + sqrt(delta) s with g_c the sign of element n + c -- per row one fma chain over c = 0 .. rank-1 from +0.0,
// then fma(sqrt(delta), s_i, chain): E[z z^T] = M exactly, for the device's own L and delta.
__device__ __forceinline__ double lpc_sign(unsigned long long seed_mixed, unsigned long long probe, unsigned long long elem)
{
    return (hash_mix64(seed_mixed ^ ((probe << 32) | elem)) >> 63) ? -1.0 : 1.0;
}

__global__ __launch_bounds__(256) void k_lpc_probes(int n, long lda, int kind, unsigned long long seed_mixed, int probe0,
                                                    const double *__restrict__ A, const double *__restrict__ L, int rank,
                                                    const LrHead *head, double *__restrict__ Z)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const unsigned long long probe = (unsigned long long)(probe0 + (int)blockIdx.y);
    const double s = lpc_sign(seed_mixed, probe, (unsigned long long)i);
    double z = s;
    if (kind == kLpcJacobi) {
        z = s * sqrt(A[i * lda + i]);
    } else if (kind == kLpcLowrank) {
        double chain = 0.0;
        for (int c = 0; c < rank; ++c) chain = fma(L[(long)c * lda + i], lpc_sign(seed_mixed, probe, (unsigned long long)n + c), chain);
        z = fma(sqrt(head->delta), s, chain);
    }
    Z[(long)blockIdx.y * lda + i] = z;
}

hipError_t launch_apply(const LanczosPcArgs &a, const double *wn, const LanczosScalars *frozen, double *wu_out, hipStream_t s)
{
    return for_multi_width(a.nvec, [&](auto w) {
        constexpr int W = decltype(w)::value;
        hipLaunchKernelGGL((k_lpc_lr_apply<W>), dim3(lr_grid(a.n)), dim3(256 * LrColsShape<W>::NG), 0, s, a.n, a.lda, a.nvec, wn, a.u, a.M.L,
                           a.M.rank, a.M.Cinv, a.M.head, a.M.tpart, frozen, a.t, wu_out);
        return hipGetLastError();
    });
}

bool lpc_args_ok(const LanczosPcArgs &a)
{
    return a.nvec >= 1 && a.nvec <= kMaxRhs && a.n >= 1 && pc_factor_ok(a.n, a.M);
}

}  // namespace

hipError_t launch_lanczos_pc_init(const LanczosPcArgs &a, hipStream_t s)
{
    if (!lpc_args_ok(a)) return hipErrorInvalidValue;
    const int g3 = multi_update_grid(a.n);
    if (a.M.dinv) {
        hipLaunchKernelGGL((k_lpc_jac_step<true>), dim3(g3, a.nvec), dim3(256), 0, s, a.n, a.lda, a.w, a.vprev, a.u, a.Y, a.M.dinv, a.k1p, a.g1,
                           a.wu_in, a.wu_out, a.ls, a.alpha, a.beta, 0);
    } else {
        hipLaunchKernelGGL((k_lpc_lr_step<true>), dim3(g3), dim3(kPcThreads), 0, s, a.n, a.lda, a.nvec, a.w, a.vprev, a.Y, a.k1p, a.g1,
                           a.wu_in, a.ls, a.alpha, a.beta, 0, a.M.L, a.M.rank, a.M.tpart);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        e = launch_apply(a, a.w, nullptr, a.wu_out, s);
        if (e != hipSuccess) return e;
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_lpc_begin, dim3(a.nvec), dim3(256), 0, s, a.wu_out, g3, a.ls);
    return hipGetLastError();
}

hipError_t launch_lanczos_pc_step(const LanczosPcArgs &a, hipStream_t s)
{
    if (!lpc_args_ok(a) || a.t < 0 || a.t >= kMaxLanczosSteps) return hipErrorInvalidValue;
    const int g3 = multi_update_grid(a.n);
    if (a.M.dinv) {
        hipLaunchKernelGGL((k_lpc_jac_step<false>), dim3(g3, a.nvec), dim3(256), 0, s, a.n, a.lda, a.w, a.vprev, a.u, a.Y, a.M.dinv, a.k1p, a.g1,
                           a.wu_in, a.wu_out, a.ls, a.alpha, a.beta, a.t);
        return hipGetLastError();
    }
    hipLaunchKernelGGL((k_lpc_lr_step<false>), dim3(g3), dim3(kPcThreads), 0, s, a.n, a.lda, a.nvec, a.w, a.vprev, a.Y, a.k1p, a.g1, a.wu_in,
                       a.ls, a.alpha, a.beta, a.t, a.M.L, a.M.rank, a.M.tpart);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_apply(a, a.vprev, a.ls, a.wu_out, s);    // w_(t+1) lies over v_(t-1)
}

hipError_t launch_lanczos_pc_close(int n, int nvec, int steps, const double *wu, LanczosScalars *ls, double *beta, hipStream_t s)
{
    if (nvec < 1 || nvec > kMaxRhs || steps < 1 || steps > kMaxLanczosSteps) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_lpc_close, dim3(nvec), dim3(256), 0, s, wu, multi_update_grid(n), steps, ls, beta);
    return hipGetLastError();
}

hipError_t launch_lanczos_pc_probes(int n, long lda, int nprobe, int kind, unsigned long long seed_mixed, int probe0, const double *A,
                                    const double *L, int rank, const LrHead *head, double *Z, hipStream_t s)
{
    if (nprobe < 1 || nprobe > kMaxRhs || n < 1 || kind < 0 || kind > kLpcLowrank) return hipErrorInvalidValue;
    if (kind == kLpcLowrank && (rank < 1 || rank > kLrMaxRank || !L || !head)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_lpc_probes, dim3(multi_update_grid(n), nprobe), dim3(256), 0, s, n, lda, kind, seed_mixed, probe0, A, L, rank, head, Z);
    return hipGetLastError();
}

}  // namespace cgx
