// cgx_shift.hip -- multi-shift CG on one GPU (cgx_solve_shifted): (A + sigma_j I) x_j = b for up to kMaxShifts shifts.
//
// The seed is the single path's recurrence on A itself from x0 = 0 (cgx_kernels.hip / cgx_symv.hip / cgx_csr.hip: K1 + K3 per
// iteration, untouched).  The residual of the shifted system stays collinear with the seed's, r^sigma_k = zeta_k r_k, so one
// pass over A per iteration serves every shift, and a shift costs a scalar recurrence and two vector updates (DESIGN.md
// section 14).  One kernel per iteration, k_shift_update, runs behind K3 of iteration k:
//
//   seed scalars   alpha_k and beta_k are stored nowhere: every workgroup refolds alpha_k from K1's p.Ap partials in K3's order
//                  and rsold, and beta_k = r_(k+1).r_(k+1) / rsold from K3's r.r partials in the order of the next K1's head
//                  (head_issue / head_finish, cgx_device.h) -- the same values added the same way, so the same bits
//   per shift      zeta_(k+1) = zeta_k zeta_(k-1) alpha_(k-1) / (alpha_k beta_(k-1) (zeta_(k-1) - zeta_k)
//                                                                  + zeta_(k-1) alpha_(k-1) (1 + sigma alpha_k))
//                  alpha^s = alpha_k zeta_(k+1) / zeta_k            x^s = fma(alpha^s, p^s, x^s)
//                  beta^s  = beta_k (zeta_(k+1) / zeta_k)^2         p^s = fma(beta^s, p^s, zeta_(k+1) * r_(k+1))
//                  with sigma = 0: zeta = 1 exactly, alpha^s = alpha, beta^s = beta, and x^s, p^s are the seed's x and p bit for bit
//   freeze         shift j is frozen in iteration k (after its x update) when |zeta_(k+1)| sqrt(r_(k+1).r_(k+1)) < tol, or when
//                  |zeta_(k+1)| < 2^-500 or is not finite (beyond a double: without the guard zeta underflows and turns into 0 / 0)
//   loop end       the seed breaks in k (sqrt(r_(k+1).r_(k+1)) < tol: what the head of K1(k+1) will find), or every shift is frozen
//
// One lane per shift advances zeta in every workgroup (the same arithmetic on the same values); workgroup 0 alone writes the
// scalar block.  What another workgroup of the same launch may still read is never overwritten: zeta and the seed's alpha / beta
// live in rings of three indexed by the iteration, and a shift's end and the loop's end are stored as the iteration number
// (ShiftScalars::frozen_at / all_at), which reads as "runs in k" before and after the store of k.
#include "cgx_kernels.h"
#include "cgx_device.h"

namespace cgx {

namespace {

constexpr double kZetaFloor = 0x1.0p-500;

// The loads of head_issue for the r.r partials, and head_finish's fold of them (every wave on its own, no LDS).
struct RrLoads {
    double a[4];
};
__device__ __forceinline__ RrLoads rr_issue(const double *__restrict__ part, int nparts)
{
    RrLoads hl;
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int t = lane + 64 * u;
        const double val = part[t < nparts ? t : nparts - 1];
        hl.a[u] = (t < nparts) ? val : 0.0;
    }
    return hl;
}
__device__ __forceinline__ double rr_finish(const RrLoads &hl, const double *__restrict__ part, int nparts)
{
    const int lane = threadIdx.x & 63;
    double v = (hl.a[0] + hl.a[1]) + (hl.a[2] + hl.a[3]);
    for (int t = lane + 256; t < nparts; t += 256) {
        const double a0 = part[t], a1 = (t + 64 < nparts) ? part[t + 64] : 0.0;
        const double a2 = (t + 128 < nparts) ? part[t + 128] : 0.0, a3 = (t + 192 < nparts) ? part[t + 192] : 0.0;
        v += (a0 + a1) + (a2 + a3);
    }
    return wave_sum(v);
}

// One workgroup of 256 threads per 256 rows (at most kMaxVectorGrid workgroups, striding above that); a thread owns a row for
// all shifts.  W = the kernel width (1, 2, 4, 8, 16 >= nshift); shifts nshift .. W-1 are masked by nshift.
// The kernel is a latency chain flag -> partials -> vectors like K3: every load of the first trip is issued before the first
// wait (the x and p of a frozen shift included: which shifts are frozen is itself a load), the stores are predicated.
template <int W>
__global__ __launch_bounds__(256) void k_shift_update(ShiftArgs a)
{
    __shared__ double lds[4];
    __shared__ double s_as[W], s_bs[W], s_zn[W];
    __shared__ int s_flag[W];                       // bit 0: x is updated, bit 1: p is updated
    const int tid = threadIdx.x, lane = tid & 63;
    const int k = a.k;
    ShiftScalars *ss = a.ss;
    const int cur = (k + 1) % 3, prv = k % 3, nxt = (k + 2) % 3;   // the ring slots of iteration k, k - 1, k + 1

    const int all_at = ss->all_at;
    const double rsold = a.sc->rs[k & 1];                          // what K3 of iteration k divided
    const int js = lane < W ? lane : W - 1;                        // the shift this lane advances (lanes >= W: discarded)
    const double zk = ss->zeta[cur][js], zm = ss->zeta[prv][js], sig = ss->sigma[js];
    const int frozen_at = ss->frozen_at[js];
    const double am = ss->alpha[prv], bm = ss->beta[prv];
    const long stride = (long)gridDim.x * 256;
    long i = (long)blockIdx.x * 256 + tid;
    const bool in = i < a.n;
    const long ic = in ? i : 0;
    const double r_i = a.r[ic];
    double xv[W], pv[W];
#pragma unroll
    for (int j = 0; j < W; ++j) {
        const long off = (long)(j < a.nshift ? j : 0) * a.lda + ic;
        xv[j] = a.X[off];
        pv[j] = a.P[off];
    }
    const RrLoads rl = rr_issue(a.rrp, a.nrr);
    // alpha_k as K3 computes it, in the order of k_update_xr or k_update_xr_strided (a loop with its own waits: behind every other load)
    const double cs = a.pap_strided ? fold_pap_strided(a.pap, 1, 0, a.npap) : fold_pap(a.pap, 1, 0, a.npap);
    if (all_at < k) return;                                        // the loop has ended (uniform over the grid): nothing is written

    const double conj = block_sum<4>(cs, lds);
    const double alpha = safeguarded_alpha(rsold, conj);           // K3's alpha_k, cg.cc:107
    const double rsnew = rr_finish(rl, a.rrp, a.nrr);              // r_(k+1).r_(k+1) as the head of K1(k+1) folds it
    const double beta = rsnew / rsold;                             // cg.cc:124
    const bool seed_break = sqrt(rsnew) < a.tol;                   // cg.cc:120-121, found by K1(k+1)

    if (tid < 64) {
        const bool live = lane < a.nshift && frozen_at >= k;
        // every operation rounded on its own, in this order (no contraction: the same bits in every width of the kernel)
        const double den = __dadd_rn(__dmul_rn(__dmul_rn(alpha, bm), __dsub_rn(zm, zk)),
                                     __dmul_rn(__dmul_rn(zm, am), __dadd_rn(1.0, __dmul_rn(sig, alpha))));
        const double zn = __ddiv_rn(__dmul_rn(__dmul_rn(zk, zm), am), den);
        const double ratio = __ddiv_rn(zn, zk);
        const double as = __dmul_rn(alpha, ratio), bs = __dmul_rn(beta, __dmul_rn(ratio, ratio));
        const double res_new = __dmul_rn(fabs(zn), sqrt(rsnew)), res_old = __dmul_rn(fabs(zk), sqrt(rsold));
        const bool finite = fabs(zn) < __builtin_inf();            // false for a NaN as well
        const bool guard = !(finite && fabs(zn) >= kZetaFloor);
        const bool freeze = live && (res_new < a.tol || guard || seed_break);
        const bool upd_x = live && finite && fabs(as) < __builtin_inf();
        const bool upd_p = live && !freeze;
        if (lane < W) {
            s_as[lane] = as;
            s_bs[lane] = bs;
            s_zn[lane] = zn;
            s_flag[lane] = (upd_x ? 1 : 0) | (upd_p ? 2 : 0);
        }
        const unsigned long long running = __ballot(upd_p);
        if (blockIdx.x == 0) {
            if (live) {
                ss->zeta[nxt][lane] = zn;
                ss->res_last[lane] = res_new;
                ss->res_prev[lane] = res_old;
                if (freeze) ss->frozen_at[lane] = k;
            }
            if (lane == 0) {
                ss->alpha[cur] = alpha;
                ss->beta[cur] = beta;
                if (running == 0) {                                // every shift is frozen, or the seed broke: the loop ends here
                    ss->all_at = k;
                    a.sc->k_final = k;                             // (what K1(k+1) writes itself where the seed broke)
                    a.sc->done = 1;
                }
            }
        }
    }
    __syncthreads();

    if (in) {
#pragma unroll
        for (int j = 0; j < W; ++j) {
            const int f = s_flag[j];
            const long off = (long)j * a.lda + i;
            if (f & 1) a.X[off] = fma(s_as[j], pv[j], xv[j]);
            if (f & 2) a.P[off] = fma(s_bs[j], pv[j], __dmul_rn(s_zn[j], r_i));   // the product rounded on its own
        }
    }
    for (i += stride; i < a.n; i += stride) {                      // more than 256 * kMaxVectorGrid rows
        const double rr = a.r[i];
#pragma unroll
        for (int j = 0; j < W; ++j) {
            const int f = s_flag[j];
            if (!f) continue;
            const long off = (long)j * a.lda + i;
            const double p = a.P[off];
            if (f & 1) a.X[off] = fma(s_as[j], p, a.X[off]);
            if (f & 2) a.P[off] = fma(s_bs[j], p, __dmul_rn(s_zn[j], rr));
        }
    }
}

// x_j = 0 and p_j = r0 = b for j < nshift (rows n .. lda-1 zero), the scalar block of iteration 0: zeta_-1 = zeta_0 = 1,
// alpha_-1 = 1, beta_-1 = 0.
__global__ __launch_bounds__(256) void k_shift_begin(int n, long lda, int nshift, ColumnSigmas sg, const double *__restrict__ b,
                                                     double *__restrict__ X, double *__restrict__ P, ShiftScalars *ss)
{
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < lda; i += (long)gridDim.x * 256) {
        const double bi = i < n ? b[i] : 0.0;
        for (int j = 0; j < nshift; ++j) {
            X[(long)j * lda + i] = 0.0;
            P[(long)j * lda + i] = bi;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < kMaxShifts) {
        const int j = threadIdx.x;
        ss->sigma[j] = j < nshift ? sg.v[j] : 0.0;
        for (int q = 0; q < 3; ++q) ss->zeta[q][j] = 1.0;
        ss->res_last[j] = ss->res_prev[j] = 0.0;
        for (int q = 0; q < 3; ++q) ss->norms[j][q] = 0.0;
        ss->frozen_at[j] = kShiftLive;
        if (j < 3) {
            ss->alpha[j] = 1.0;
            ss->beta[j] = 0.0;
        }
        if (j == 0) ss->all_at = kShiftLive;
    }
}

// The loop ran out after k iterations (one wave): a shift that is still running reports |zeta_k| sqrt(r_k.r_k) as both residuals,
// as the seed does when its loop runs out (cg.cc:132: rsold = rsnew); k == 0: nothing ran, that is sqrt(r0.r0).
__global__ __launch_bounds__(64) void k_shift_close(ShiftScalars *ss, const double *__restrict__ rrp, int nrr, int nshift, int k)
{
    const int lane = threadIdx.x;
    const double rs0 = rr_finish(rr_issue(rrp, nrr), rrp, nrr);
    if (lane >= nshift || ss->frozen_at[lane] != kShiftLive) return;
    if (k == 0) ss->res_last[lane] = sqrt(rs0);
    ss->res_prev[lane] = ss->res_last[lane];
}

}  // namespace

hipError_t launch_shift_begin(int n, long lda, int nshift, const double *sigma, const double *b, double *X, double *P, ShiftScalars *ss,
                              hipStream_t s)
{
    if (nshift < 1 || nshift > kMaxShifts || n < 1 || lda < n) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_shift_begin, dim3(update_xr_grid((int)lda)), dim3(256), 0, s, n, lda, nshift, column_sigmas(sigma, nshift), b, X,
                       P, ss);
    return hipGetLastError();
}

hipError_t launch_shift_update(const ShiftArgs &a, hipStream_t s)
{
    if (a.nshift < 1 || a.nshift > kMaxShifts || a.n < 1 || a.lda < a.n || a.nrr < 1 || a.npap < 1) return hipErrorInvalidValue;
    const dim3 grid(update_xr_grid(a.n)), block(256);
    for_multi_width(a.nshift, [&](auto w) { hipLaunchKernelGGL(k_shift_update<decltype(w)::value>, grid, block, 0, s, a); });
    return hipGetLastError();
}

hipError_t launch_shift_close(ShiftScalars *ss, const double *rrp, int nrr, int nshift, int k, hipStream_t s)
{
    if (nshift < 1 || nshift > kMaxShifts || nrr < 1 || k < 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_shift_close, dim3(1), dim3(64), 0, s, ss, rrp, nrr, nshift, k);
    return hipGetLastError();
}

}  // namespace cgx
