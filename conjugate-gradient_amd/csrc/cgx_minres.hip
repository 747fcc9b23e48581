// cgx_minres.hip -- MINRES on one GPU (cgx_solve_minres): (A + sigma_j I) x_j = b for up to kMaxMinresShifts shifts of either sign,
// A symmetric and not necessarily definite.
//
// The Lanczos recurrence from r0 = b does not depend on the shift, so one pass over A per iteration serves every shift:
//
//   beta_0 = ||b||, v_0 = b / beta_0, v_-1 = 0
//   step t:    y = A v_t;  alpha_t = v_t . y;  w = y - alpha_t v_t - beta_t v_(t-1);  beta_(t+1) = ||w||;  v_(t+1) = w / beta_(t+1)
//   column t of T + sigma_j I is (beta_t, alpha_t + sigma_j, beta_(t+1)): the two previous rotations and a new one (c, s) reduce
//   it to (eps, delta, gamma) (Paige and Saunders 1975);  d_t = (v_t - delta d_(t-1) - eps d_(t-2)) / gamma;
//   x += phi d_t with phi = c phibar, phibar <- s phibar from phibar = beta_0;  |phibar| = ||(A + sigma_j I) x_j - b||
//
// The mat-vec is the plain K1 of the shard's plan (cgx_kernels.hip / cgx_symv.hip / cgx_csr.hip, untouched), run as in
// cgx_lanczos.hip on the NOT YET NORMALISED w_t: it leaves Y = A w_t and the partials of w_t . A w_t.  k_minres_step does the rest
// of launch t: beta_t from the ||w_t||^2 partials of launch t - 1, alpha_t = (w_t . A w_t) / ||w_t||^2, the breakdown test
// beta_t <= 2^-36 max |alpha|, and per row v_t = w / beta_t (over w) and w_(t+1) = Y / beta_t - alpha_t v_t - beta_t v_(t-1) (over
// v_(t-1)) with one ||w_(t+1)||^2 partial per workgroup.  Column t - 1 needed beta_t, so it is closed in the same launch, one
// lane per shift, and the x update lags the recurrence by one launch: v_(t-1) is the vector this launch reads anyway.  The close
// kernel applies the last column.
//
// Every workgroup folds the same partials in the same fixed order (fold_pap + block_sum<4>) and advances every shift with the
// same arithmetic, each operation rounded on its own, so every width of the kernel gives the same bits; workgroup 0 alone writes
// the scalar block, into the parity slots no workgroup of the same launch reads, and a shift's end and the loop's end are stored
// as numbers (MinresScalars::frozen_at / end_at) that read as "running" before and after the store.  No floating-point atomics.
#include "cgx_kernels.h"
#include "cgx_device.h"

namespace cgx {

namespace {

constexpr double kMinresBreak = 0x1.0p-36;   // cgx_lanczos.hip's rule: beta <= 2^-36 max |alpha| ends the recurrence
constexpr double kDblMax = 1.7976931348623157e308;

// What the lane of shift j loads of the scalar block in front of column k (slot (k + 1) & 1).
struct MinresLane {
    double cs, sn, dbar, eps, phibar, sigma;
    int frozen_at;
};
__device__ __forceinline__ MinresLane lane_load(const MinresScalars *ms, int slot, int j)
{
    return MinresLane{ms->cs[slot][j], ms->sn[slot][j], ms->dbar[slot][j], ms->eps[slot][j], ms->phibar[slot][j], ms->sigma[j],
                      ms->frozen_at[j]};
}

// Column k of shift `lane` (wave 0 of every workgroup, all 64 lanes): (beta_k, alpha_k + sigma, bnext) with bnext = beta_(k+1), or 0
// where the recurrence broke down there.  Leaves (delta, eps, gamma, phi) and the shift's update flag in LDS for the rows; the
// writer (workgroup 0) stores the state in front of column k + 1 into slot wr, the residuals and the shift's end.  Returns the
// ballot of the shifts still running behind this column.  Every operation is rounded on its own: no contraction, the same bits
// in every kernel that calls this.
__device__ __forceinline__ unsigned long long minres_column(MinresScalars *ms, const MinresLane &q, int lane, int width, int nshift,
                                                            int k, int wr, double alpha_k, double bnext, bool breakdown, double amax,
                                                            double tol, bool writer, double *s_del, double *s_eps, double *s_gam,
                                                            double *s_phi, int *s_flag)
{
    const bool live = lane < nshift && q.frozen_at >= k;
    const double alfa = __dadd_rn(alpha_k, q.sigma);
    const double delta = __dadd_rn(__dmul_rn(q.cs, q.dbar), __dmul_rn(q.sn, alfa));
    const double gbar = __dsub_rn(__dmul_rn(q.sn, q.dbar), __dmul_rn(q.cs, alfa));   // the diagonal in front of the new rotation
    const double eps_n = __dmul_rn(q.sn, bnext), dbar_n = -__dmul_rn(q.cs, bnext);
    const double gamma = __dsqrt_rn(__dadd_rn(__dmul_rn(gbar, gbar), __dmul_rn(bnext, bnext)));
    const double cs_n = __ddiv_rn(gbar, gamma), sn_n = __ddiv_rn(bnext, gamma);
    const double phi = __dmul_rn(cs_n, q.phibar), phibar_n = __dmul_rn(sn_n, q.phibar);
    const double res_old = fabs(q.phibar), res_new = fabs(phibar_n);
    const bool finite = fabs(gamma) < __builtin_inf() && fabs(phi) < __builtin_inf();   // false for a NaN as well
    const bool singular = breakdown && fabs(gbar) <= __dmul_rn(kMinresBreak, __dadd_rn(amax, fabs(q.sigma)));
    const bool upd = live && finite && !singular;
    const bool conv = upd && (breakdown || res_new < tol);
    const bool freeze = live && (!upd || conv);
    if (lane < width) {
        s_del[lane] = delta;
        s_eps[lane] = q.eps;
        s_gam[lane] = gamma;
        s_phi[lane] = phi;
        s_flag[lane] = upd ? 1 : 0;
    }
    if (writer && live) {
        ms->cs[wr][lane] = cs_n;
        ms->sn[wr][lane] = sn_n;
        ms->dbar[wr][lane] = dbar_n;
        ms->eps[wr][lane] = eps_n;
        ms->phibar[wr][lane] = phibar_n;
        ms->res_prev[lane] = res_old;
        ms->res_last[lane] = upd ? (breakdown ? 0.0 : res_new) : res_old;
        if (freeze) {
            ms->frozen_at[lane] = k;
            ms->conv[lane] = conv ? 1 : 0;
        }
    }
    return __ballot(live && !freeze);
}

// d_(k) = (v_k - delta d_(k-1) - eps d_(k-2)) / gamma
__device__ __forceinline__ double minres_dir(double u, double del, double d1, double eps, double d2, double gam)
{
    return __ddiv_rn(fma(-eps, d2, fma(-del, d1, u)), gam);
}

// One workgroup of 256 threads per 256 rows (at most kMaxVectorGrid workgroups, striding above that); a thread owns a row for the
// recurrence and all shifts: 3 + 3 W doubles live.  W = the kernel width (1, 2, 4, 8, 16 >= nshift); shifts nshift .. W-1 are
// masked by nshift.  A latency chain partials -> scalars -> vectors like K3: every load of the first trip is issued before the
// first wait (the x and d of a frozen shift included: which shifts are frozen is itself a load), the stores are predicated.
template <int W>
__global__ __launch_bounds__(256) void k_minres_step(MinresArgs a)
{
    __shared__ double lds[4];
    __shared__ double s_del[W], s_eps[W], s_gam[W], s_phi[W];
    __shared__ int s_flag[W];
    const int tid = threadIdx.x, lane = tid & 63;
    const int t = a.t, rd = t & 1, wr = rd ^ 1;
    MinresScalars *ms = a.ms;

    const int end_at = ms->end_at;
    const int js = lane < W ? lane : W - 1;                        // the shift this lane advances (lanes >= W: discarded)
    const MinresLane q = lane_load(ms, rd, js);
    const double alpha_m = ms->alpha[wr], amax = ms->amax[wr];     // alpha_(t-1), max |alpha_s| over s <= t - 1
    double *const d1p = a.D[rd], *const d2p = a.D[wr];             // d_(t-2); d_(t-3), which d_(t-1) replaces
    const long stride = (long)gridDim.x * 256;
    long i = (long)blockIdx.x * 256 + tid;
    const bool in = i < a.n;
    const long ic = in ? i : 0;
    const double w_i = a.w[ic], y_i = a.Y[ic], u_i = a.vprev[ic];
    double xv[W], d1v[W], d2v[W];
#pragma unroll
    for (int j = 0; j < W; ++j) {
        const long off = (long)(j < a.nshift ? j : 0) * a.lda + ic;
        xv[j] = a.X[off];
        d1v[j] = d1p[off];
        d2v[j] = d2p[off];
    }
    const double ws = fold_pap(a.ww_in, 1, 0, (int)gridDim.x);
    const double cs = fold_pap(a.k1p, 1, 0, a.nk1p);
    if (end_at < t) return;                                        // the loop has ended (uniform over the grid): nothing is written

    const double ww = block_sum<4>(ws, lds);                       // ||w_t||^2
    const double wAw = block_sum<4>(cs, lds);                      // w_t . A w_t
    const double beta = sqrt(ww);                                  // beta_t
    const double alpha = __ddiv_rn(wAw, ww);                       // alpha_t
    // t = 0: b = 0 (x = 0 solves every system) or b not finite; t > 0: an invariant subspace
    const bool breakdown = t == 0 ? !(ww > 0.0 && ww <= kDblMax) : beta <= __dmul_rn(kMinresBreak, amax);
    const bool writer = blockIdx.x == 0;

    if (tid < 64) {
        unsigned long long running = 0;
        if (t > 0) {
            running = minres_column(ms, q, lane, W, a.nshift, t - 1, wr, alpha_m, breakdown ? 0.0 : beta, breakdown, amax, a.tol, writer,
                                    s_del, s_eps, s_gam, s_phi, s_flag);
        } else {
            if (lane < W) s_flag[lane] = 0;
            if (writer && lane < a.nshift) {                       // the state in front of column 0: no rotation yet, phibar = beta_0
                ms->cs[wr][lane] = -1.0;
                ms->sn[wr][lane] = 0.0;
                ms->dbar[wr][lane] = 0.0;
                ms->eps[wr][lane] = 0.0;
                ms->phibar[wr][lane] = beta;
                ms->res_last[lane] = ms->res_prev[lane] = beta;
                if (breakdown) {
                    ms->frozen_at[lane] = 0;
                    ms->conv[lane] = ww == 0.0 ? 1 : 0;
                }
            }
            running = breakdown ? 0 : 1;
        }
        if (writer && lane == 0) {
            if (!breakdown) {
                const double aa = fabs(alpha);
                ms->alpha[rd] = alpha;
                ms->amax[rd] = aa > amax ? aa : amax;
            }
            if (running == 0 || breakdown) {                       // every shift is frozen, or the recurrence ended: the loop ends here
                ms->end_at = t;
                ms->done = 1;
            }
        }
    }
    __syncthreads();

    double nw = 0.0;
    if (in) {
        if (!breakdown) {
            const double v = __ddiv_rn(w_i, beta), y = __ddiv_rn(y_i, beta);
            const double wn = fma(-beta, u_i, fma(-alpha, v, y));
            a.w[i] = v;
            a.vprev[i] = wn;
            nw = __dmul_rn(wn, wn);
        }
#pragma unroll
        for (int j = 0; j < W; ++j) {
            if (!s_flag[j]) continue;
            const long off = (long)j * a.lda + i;
            const double dn = minres_dir(u_i, s_del[j], d1v[j], s_eps[j], d2v[j], s_gam[j]);
            d2p[off] = dn;
            a.X[off] = fma(s_phi[j], dn, xv[j]);
        }
    }
    for (i += stride; i < a.n; i += stride) {                      // more than 256 * kMaxVectorGrid rows
        const double u = a.vprev[i];
        if (!breakdown) {
            const double v = __ddiv_rn(a.w[i], beta), y = __ddiv_rn(a.Y[i], beta);
            const double wn = fma(-beta, u, fma(-alpha, v, y));
            a.w[i] = v;
            a.vprev[i] = wn;
            nw = fma(wn, wn, nw);
        }
#pragma unroll
        for (int j = 0; j < W; ++j) {
            if (!s_flag[j]) continue;
            const long off = (long)j * a.lda + i;
            const double dn = minres_dir(u, s_del[j], d1p[off], s_eps[j], d2p[off], s_gam[j]);
            d2p[off] = dn;
            a.X[off] = fma(s_phi[j], dn, a.X[off]);
        }
    }
    nw = block_sum<4>(nw, lds);
    if (tid == 0) a.ww_out[blockIdx.x] = nw;
}

// The grid of the step kernel, so that the ||b||^2 partials are the ones its launch 0 folds.
__global__ __launch_bounds__(256) void k_minres_init(MinresArgs a, ColumnSigmas sg, const double *__restrict__ b)
{
    __shared__ double lds[4];
    double bb = 0.0;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < a.lda; i += (long)gridDim.x * 256) {
        const double bi = i < a.n ? b[i] : 0.0;
        a.w[i] = bi;
        a.vprev[i] = 0.0;
        bb = fma(bi, bi, bb);
        for (int j = 0; j < a.nshift; ++j) {
            const long off = (long)j * a.lda + i;
            a.X[off] = 0.0;
            a.D[0][off] = 0.0;
            a.D[1][off] = 0.0;
        }
    }
    bb = block_sum<4>(bb, lds);
    if (threadIdx.x == 0) a.ww_out[blockIdx.x] = bb;
    if (blockIdx.x == 0 && threadIdx.x < kMaxMinresShifts) {
        const int j = threadIdx.x;
        MinresScalars *ms = a.ms;
        ms->sigma[j] = j < a.nshift ? sg.v[j] : 0.0;
        for (int q = 0; q < 2; ++q) {
            ms->cs[q][j] = -1.0;
            ms->sn[q][j] = ms->dbar[q][j] = ms->eps[q][j] = ms->phibar[q][j] = 0.0;
        }
        ms->res_last[j] = ms->res_prev[j] = 0.0;
        ms->frozen_at[j] = kMinresLive;
        ms->conv[j] = 0;
        if (j < 2) ms->alpha[j] = ms->amax[j] = 0.0;
        if (j == 0) {
            ms->done = 0;
            ms->end_at = kMinresLive;
        }
    }
}

// The loop ran out after k = a.t launches: column k - 1 still waits for beta_k, which the last launch left as partials.  The step
// kernel's grid and the step kernel's arithmetic (minres_column, minres_dir) at full width, the shifts in a loop.  k == 0: nothing
// ran, and both residuals are ||b||.
__global__ __launch_bounds__(256) void k_minres_close(MinresArgs a)
{
    constexpr int W = kMaxMinresShifts;
    __shared__ double lds[4];
    __shared__ double s_del[W], s_eps[W], s_gam[W], s_phi[W];
    __shared__ int s_flag[W];
    const int tid = threadIdx.x, lane = tid & 63;
    const int k = a.t, rd = k & 1, wr = rd ^ 1;
    MinresScalars *ms = a.ms;
    const int end_at = ms->end_at;
    const int js = lane < W ? lane : W - 1;
    const MinresLane q = lane_load(ms, rd, js);
    const double alpha_m = ms->alpha[wr], amax = ms->amax[wr];
    const double ws = fold_pap(a.ww_in, 1, 0, (int)gridDim.x);
    if (end_at != kMinresLive) return;
    const double ww = block_sum<4>(ws, lds);
    const double beta = sqrt(ww);
    const bool writer = blockIdx.x == 0;
    if (k == 0) {
        if (writer && tid < a.nshift) ms->res_last[tid] = ms->res_prev[tid] = beta;
        return;
    }
    const bool breakdown = beta <= __dmul_rn(kMinresBreak, amax);
    if (tid < 64)
        (void)minres_column(ms, q, lane, W, a.nshift, k - 1, wr, alpha_m, breakdown ? 0.0 : beta, breakdown, amax, a.tol, writer, s_del,
                            s_eps, s_gam, s_phi, s_flag);
    __syncthreads();
    double *const d1p = a.D[rd], *const d2p = a.D[wr];
    for (long i = (long)blockIdx.x * 256 + tid; i < a.n; i += (long)gridDim.x * 256) {
        const double u = a.vprev[i];
        for (int j = 0; j < a.nshift; ++j) {
            if (!s_flag[j]) continue;
            const long off = (long)j * a.lda + i;
            const double dn = minres_dir(u, s_del[j], d1p[off], s_eps[j], d2p[off], s_gam[j]);
            d2p[off] = dn;
            a.X[off] = fma(s_phi[j], dn, a.X[off]);
        }
    }
}

bool args_ok(const MinresArgs &a)
{
    return a.nshift >= 1 && a.nshift <= kMaxMinresShifts && a.n >= 1 && a.lda >= a.n && a.t >= 0;
}

}  // namespace

hipError_t launch_minres_init(const MinresArgs &a, const double *sigma, const double *b, hipStream_t s)
{
    if (!args_ok(a)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_minres_init, dim3(update_xr_grid(a.n)), dim3(256), 0, s, a, column_sigmas(sigma, a.nshift), b);
    return hipGetLastError();
}

hipError_t launch_minres_step(const MinresArgs &a, hipStream_t s)
{
    if (!args_ok(a) || a.nk1p < 1) return hipErrorInvalidValue;
    const dim3 grid(update_xr_grid(a.n)), block(256);
    for_multi_width(a.nshift, [&](auto w) { hipLaunchKernelGGL(k_minres_step<decltype(w)::value>, grid, block, 0, s, a); });
    return hipGetLastError();
}

hipError_t launch_minres_close(const MinresArgs &a, hipStream_t s)
{
    if (!args_ok(a)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_minres_close, dim3(update_xr_grid(a.n)), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace cgx
