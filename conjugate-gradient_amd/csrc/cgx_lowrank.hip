// cgx_lowrank.hip -- the pivoted-Cholesky low-rank preconditioner, one GPU, dense storage:
//   A ~ L L^T + delta I  (L: n x rank, partial Cholesky with diagonal pivoting),  z = P^-1 r = (r - L C^-1 L^T r) / delta,
//   C = delta I + L^T L  (rank x rank, inverted once per matrix by block Jacobi's symmetric sweep, launch_bj_invert).
// L is column-major at the matrix pitch (L[u * lda + i], zero in the pad rows), like block Jacobi's W: every load of the loop is
// coalesced over rows.  Set-up: k_lr_init, one k_lr_step per column, k_lr_delta, k_lr_gram; loop: k_lr_update (the PCG update
// kernel of section 11 plus one partial of t = L^T r per workgroup and column) and k_lr_apply (fold t, u = C^-1 t, z, r.z).
// No floating-point atomics; every sum has a fixed order, so a solve repeats bit for bit.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <climits>
#include <cmath>

#include "cgx_lowrank_cols.h"

namespace cgx {

namespace {

constexpr double kLrMax = 1.7976931348623157e308;

// ---- the pivot search: the largest remaining diagonal, ties to the smallest index ---------------------------------------------
// (v, i) pairs are totally ordered (a retired or missing row carries -inf, a NaN is turned into -inf before it gets here), so the
// result does not depend on the order of the fold; the order is fixed all the same.
__device__ __forceinline__ void lr_better(double &v, int &i, double v2, int i2)
{
    if (v2 > v || (v2 == v && i2 < i)) {
        v = v2;
        i = i2;
    }
}

__device__ __forceinline__ double lr_sane(double v) { return v > -HUGE_VAL ? v : -HUGE_VAL; }   // NaN -> -inf

// the workgroup's best pair, in every thread
__device__ __forceinline__ void lr_block_best(double &v, int &i, double *lv /* 4 */, int *li /* 4 */)
{
#pragma unroll
    for (int w = 32; w >= 1; w >>= 1) {
        const double v2 = __shfl_xor(v, w, 64);
        const int i2 = __shfl_xor(i, w, 64);
        lr_better(v, i, v2, i2);
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    __syncthreads();   // protect lv / li against a previous use
    if (lane == 0) {
        lv[wv] = v;
        li[wv] = i;
    }
    __syncthreads();
    v = lv[0];
    i = li[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) lr_better(v, i, lv[w], li[w]);
}

// sum_u col[u * stride] * vec[u] for u = 0 ... count-1: ONE fma chain from +0.0 in ascending u, DEPTH loads in flight (the chain
// is a string of memory round trips; what it costs is their number, not the arithmetic).  The last trip is a full one too: its
// columns past count are clamped to the last one and meet vec's zeros (vec holds zeros from count up to the next multiple of
// DEPTH), so they leave the sum as it is.
template <int DEPTH>
__device__ __forceinline__ double lr_chain(const double *__restrict__ col, long stride, const double *vec, int count)
{
    double acc = 0.0;
    for (int u = 0; u < count; u += DEPTH) {
        double w[DEPTH];
#pragma unroll
        for (int q = 0; q < DEPTH; ++q) w[q] = col[(long)(u + q < count ? u + q : count - 1) * stride];
#pragma unroll
        for (int q = 0; q < DEPTH; ++q) acc = fma(w[q], vec[u + q], acc);
    }
    return acc;
}

__device__ __forceinline__ bool lr_failed(const LrHead *h) { return h->bad_step != kLrArmed || h->bad_row != kLrArmed; }

}  // namespace

// ---- set-up ---------------------------------------------------------------------------------------------------------------------
// d = diag(A); a diagonal entry that is not finite and > 0 lowers head->bad_row to its row (the head is armed by the host: every
// int kLrArmed); candidate of every tile of 256 rows for step 0.
__global__ __launch_bounds__(256) void k_lr_init(const double *__restrict__ A, long lda, int n, double *__restrict__ d,
                                                  double *__restrict__ cand_v, int *__restrict__ cand_i, LrHead *head)
{
    __shared__ double lv[4];
    __shared__ int li[4];
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    double v = -HUGE_VAL;
    int idx = INT_MAX;
    if (i < n) {
        const double dv = A[(long)i * lda + i];
        d[i] = dv;
        if (!(dv > 0.0 && dv <= kLrMax)) atomicMin(&head->bad_row, i);
        v = lr_sane(dv);
        idx = i;
    }
    lr_block_best(v, idx, lv, li);
    if (threadIdx.x == 0) {
        cand_v[blockIdx.x] = v;
        cand_i[blockIdx.x] = idx;
    }
}

// Step t: every workgroup folds the G candidates of the previous step (cv_in / ci_in; this launch writes the other pair), takes
// the pivot p with remaining diagonal pv, then for its 256 rows: column t of L, the remaining diagonal, the next candidate.
__global__ __launch_bounds__(256) void k_lr_step(const double *__restrict__ A, long lda, int n, int t, double *__restrict__ L,
                                                  double *__restrict__ d, const double *__restrict__ cv_in,
                                                  const int *__restrict__ ci_in, double *__restrict__ cv_out, int *__restrict__ ci_out,
                                                  int G, int *__restrict__ piv, LrHead *head)
{
    __shared__ double lv[4];
    __shared__ int li[4];
    __shared__ double lp[kLrMaxRank];
    const int tid = (int)threadIdx.x;
    double pv = -HUGE_VAL;
    int p = INT_MAX;
    for (int g = tid; g < G; g += 256) lr_better(pv, p, cv_in[g], ci_in[g]);
    lr_block_best(pv, p, lv, li);
    // an earlier step (or the diagonal check) failed, or this pivot is not finite and > 0: the same decision in every workgroup
    const bool ok = pv > 0.0 && pv <= kLrMax && p >= 0 && p < n;
    if (lr_failed(head)) return;
    if (!ok) {
        if (blockIdx.x == 0 && tid == 0) {
            head->bad_step = t;
            head->bad_row = (p >= 0 && p < n) ? p : -1;
        }
        return;
    }
    if (blockIdx.x == 0 && tid == 0) piv[t] = p;
    lp[tid] = tid < t ? L[(long)tid * lda + p] : 0.0;   // row p of the columns made so far, zeros behind them
    __syncthreads();
    const int i = (int)blockIdx.x * 256 + tid;
    double v = -HUGE_VAL;
    int idx = INT_MAX;
    if (i < n) {
        const double di = d[i];
        const double a = A[(long)p * lda + i];        // the pivot's ROW of A: coalesced (A is symmetric)
        double *Li = L + i;
        const double acc = lr_chain<16>(Li, lda, lp, t);
        const double sq = sqrt(pv);
        const bool retired = di == -HUGE_VAL;         // chosen at an earlier step
        double l = (a - acc) / sq;
        double dn = fma(-l, l, di);
        if (i == p) {
            l = sq;
            dn = -HUGE_VAL;
        } else if (retired) {
            l = 0.0;
            dn = -HUGE_VAL;
        }
        Li[(long)t * lda] = l;
        d[i] = dn;
        v = lr_sane(dn);
        idx = i;
    }
    lr_block_best(v, idx, lv, li);
    if (tid == 0) {
        cv_out[blockIdx.x] = v;
        ci_out[blockIdx.x] = idx;
    }
}

// delta: the given shift, or (sum of the remaining diagonal) / n -- one workgroup, thread-strided sums, then the block fold.
__global__ __launch_bounds__(256) void k_lr_delta(const double *__restrict__ d, int n, double shift, LrHead *head)
{
    __shared__ double lds[4];
    if (lr_failed(head)) return;
    double delta = shift;
    if (!(shift > 0.0)) {
        double s = 0.0;
        for (int i = (int)threadIdx.x; i < n; i += 256) {
            const double di = d[i];
            s += di == -HUGE_VAL ? 0.0 : di;
        }
        delta = block_sum<4>(s, lds) / (double)n;
    }
    if (threadIdx.x == 0) {
        head->delta = delta;
        head->delta_bad = (delta > 0.0 && delta <= kLrMax) ? 0 : 1;
    }
}

// C = delta I + L^T L, pitch kLrLd.  Workgroup (bu, bv), bu <= bv, owns the 8 x 8 entries (8 bu + q, 8 bv + s): every thread
// strides over the rows with 64 accumulators, then one wave fold per entry and the four waves in order; both triangles stored.
__global__ __launch_bounds__(256) void k_lr_gram(const double *__restrict__ L, long lda, int n, int rank, const LrHead *head,
                                                  double *__restrict__ C)
{
    __shared__ double part[4][64];
    const int bu = (int)blockIdx.x, bv = (int)blockIdx.y;
    if (bu > bv || lr_failed(head) || head->delta_bad) return;
    const double *ca[8], *cb[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {                     // columns past the rank: clamped here, never stored below
        const int ua = 8 * bu + q, ub = 8 * bv + q;
        ca[q] = L + (long)(ua < rank ? ua : rank - 1) * lda;
        cb[q] = L + (long)(ub < rank ? ub : rank - 1) * lda;
    }
    double acc[8][8];
#pragma unroll
    for (int q = 0; q < 8; ++q)
#pragma unroll
        for (int s = 0; s < 8; ++s) acc[q][s] = 0.0;
    for (int i = (int)threadIdx.x; i < n; i += 256) {
        double a[8], b[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            a[q] = ca[q][i];
            b[q] = cb[q][i];
        }
#pragma unroll
        for (int q = 0; q < 8; ++q)
#pragma unroll
            for (int s = 0; s < 8; ++s) acc[q][s] = fma(a[q], b[s], acc[q][s]);
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < 8; ++q)
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            const double tot = wave_sum(acc[q][s]);
            if (lane == 0) part[w][q * 8 + s] = tot;
        }
    __syncthreads();
    if (threadIdx.x < 64) {
        const int e = (int)threadIdx.x, u = 8 * bu + e / 8, v = 8 * bv + e % 8;
        if (u < rank && v < rank) {
            double c = ((part[0][e] + part[1][e]) + part[2][e]) + part[3][e];
            if (u == v) c += head->delta;
            C[(long)u * kLrLd + v] = c;
            C[(long)v * kLrLd + u] = c;
        }
    }
}

// ---- the loop -------------------------------------------------------------------------------------------------------------------
// The update kernel: k_update_xr_pc's loads, fold of p.Ap and alpha (K3's order), x += alpha p, r -= alpha Ap, the r.r partial
// behind z's r.z partials -- and, with the tile's r in LDS, tpart[wg][u] = sum over the tile of L[i][u] r_i: the columns go over
// the waves in groups of eight (32 loads in flight per lane), one 8-row wave fold per group.  INIT: r is taken as it is (set-up from x0, and the probe).
template <bool INIT>
__global__ __launch_bounds__(256) void k_lr_update(int n, const double *__restrict__ p_new, SegView apv, int tail_count,
                                                    double *__restrict__ x, double *r, Scalars *sc, int parity,
                                                    const double *__restrict__ L, long lda, int rank, SegView zv,
                                                    double *__restrict__ tpart)
{
    __shared__ double lds[4];
    __shared__ double rl[256];
    const int tid = (int)threadIdx.x;
    const int base = (int)blockIdx.x * 256;
    const int i = base + tid;
    const bool in = i < n;
    double rn = 0.0;
    if constexpr (INIT) {
        if (in) rn = r[i];
    } else {
        const int done = sc->done;
        const double rsold = sc->rs[parity];
        double ap_i = 0.0, r_i = 0.0, p_i = 0.0, x_i = 0.0;
        if (in) {
            ap_i = apv.base[i];
            r_i = r[i];
            p_i = p_new[i];
            x_i = x[i];
        }
        const double cs = fold_pap(apv.base + apv.Sr, 1, 0, tail_count);
        if (done) return;   // converged earlier (uniform over the grid): nothing is written
        const double conj = block_sum<4>(cs, lds);
        const double alpha = safeguarded_alpha(rsold, conj);   // alpha = rho / p.Ap
        if (in) {
            rn = fma(-alpha, ap_i, r_i);
            r[i] = rn;
            x[i] = fma(alpha, p_i, x_i);
        }
    }
    rl[tid] = rn;   // rows past n: exactly 0
    const double rr = block_sum<4>(rn * rn, lds);   // (its barriers also publish rl)
    if (tid == 0) zv.base[zv.S + blockIdx.x] = rr;
    const int lane = tid & 63, w = tid >> 6;
    const int last = n - 1 - base;                  // >= 0: the grid has no workgroup past n
    int ro[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) ro[q] = (lane + 64 * q) <= last ? lane + 64 * q : last;   // clamped: r is 0 there
    double rq[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) rq[q] = rl[lane + 64 * q];
    for (int g = w; 8 * g < rank; g += 4) {
        double v[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const int u = 8 * g + c;
            const double *col = L + (long)(u < rank ? u : rank - 1) * lda + base;
            double s = 0.0;
#pragma unroll
            for (int q = 0; q < 4; ++q) s = fma(col[ro[q]], rq[q], s);
            v[c] = u < rank ? s : 0.0;
        }
        const int row = wave_sum_rows<8>(v, lane);
        if ((lane & 7) == 0 && 8 * g + row < rank) tpart[(long)blockIdx.x * kLrLd + 8 * g + row] = v[0];
    }
}

// The apply kernel: every workgroup folds the G partials of t in ascending workgroup order, forms u = C^-1 t (one fma chain per
// entry, ascending), then z_i = (r_i - sum_u L[i][u] u_u) / delta for its rows and the r.z partial in z's tail.
__global__ __launch_bounds__(256) void k_lr_apply(int n, const double *__restrict__ r, const double *__restrict__ L, long lda,
                                                   int rank, const double *__restrict__ Cinv, const LrHead *head,
                                                   const double *__restrict__ tpart, int G, const Scalars *sc, SegView zv)
{
    __shared__ double lds[4];
    __shared__ double ts[kLrMaxRank];
    __shared__ double us[kLrMaxRank];
    const int tid = (int)threadIdx.x;
    if (sc && sc->done) return;   // converged earlier (uniform): z and its partials stay as they are
    const double delta = head->delta;
    const int i = (int)blockIdx.x * 256 + tid;
    const bool in = i < n;
    const double r_i = in ? r[i] : 0.0;
    const double t = lr_fold_tiles(tpart + (tid < rank ? tid : 0), G);
    ts[tid] = tid < rank ? t : 0.0;   // zeros behind the rank: lr_chain's last trip
    __syncthreads();
    // C^-1 is symmetric bit for bit: row tid read as column tid, coalesced
    us[tid] = tid < rank ? lr_chain<16>(Cinv + tid, kLrLd, ts, rank) : 0.0;
    __syncthreads();
    double rz = 0.0;
    if (in) {
        const double s = lr_chain<16>(L + i, lda, us, rank);
        const double z = (r_i - s) / delta;
        zv.base[i] = z;
        rz = r_i * z;
    }
    rz = block_sum<4>(rz, lds);
    if (tid == 0) zv.base[zv.Sr + blockIdx.x] = rz;
}

// ---- launchers ------------------------------------------------------------------------------------------------------------------
int lr_grid(int n) { return (n + 255) / 256; }

bool pc_factor_ok(int n, const PcFactor &f)
{
    if (f.dinv) return true;
    const int g3 = multi_update_grid(n);
    return f.rank >= 1 && f.rank <= kLrMaxRank && f.rank <= n && g3 == lr_grid(n) && g3 <= kMaxVectorGrid;
}

hipError_t launch_lr_init(const double *A, long lda, int n, const LrWork &w, hipStream_t s)
{
    hipLaunchKernelGGL(k_lr_init, dim3(lr_grid(n)), dim3(256), 0, s, A, lda, n, w.d, w.cand_v, w.cand_i, w.head);
    return hipGetLastError();
}

hipError_t launch_lr_step(const double *A, long lda, int n, int t, double *L, const LrWork &w, hipStream_t s)
{
    if (t < 0 || t >= kLrMaxRank) return hipErrorInvalidValue;
    const int G = lr_grid(n), in = t & 1, out = in ^ 1;
    hipLaunchKernelGGL(k_lr_step, dim3(G), dim3(256), 0, s, A, lda, n, t, L, w.d, w.cand_v + in * kMaxVectorGrid,
                       w.cand_i + in * kMaxVectorGrid, w.cand_v + out * kMaxVectorGrid, w.cand_i + out * kMaxVectorGrid, G, w.piv,
                       w.head);
    return hipGetLastError();
}

hipError_t launch_lr_finish(const double *L, long lda, int n, int rank, double shift, const LrWork &w, hipStream_t s)
{
    if (rank < 1 || rank > kLrMaxRank) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_lr_delta, dim3(1), dim3(256), 0, s, w.d, n, shift, w.head);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const int nb = (rank + 7) / 8;
    hipLaunchKernelGGL(k_lr_gram, dim3(nb, nb), dim3(256), 0, s, L, lda, n, rank, w.head, w.C);
    return hipGetLastError();
}

hipError_t launch_lr_update(int n, const double *p_new, SegView apv, int tail_count, double *x, double *r, Scalars *sc, int parity,
                            const double *L, long lda, int rank, SegView zv, const LrWork &w, hipStream_t s, hipEvent_t e0,
                            hipEvent_t e1)
{
    hipExtLaunchKernelGGL((k_lr_update<false>), dim3(lr_grid(n)), dim3(256), 0, s, e0, e1, 0, n, p_new, apv, tail_count, x, r, sc,
                          parity, L, lda, rank, zv, w.tpart);
    return hipGetLastError();
}

hipError_t launch_lr_update_init(int n, double *r, const double *L, long lda, int rank, SegView zv, const LrWork &w, hipStream_t s)
{
    hipLaunchKernelGGL((k_lr_update<true>), dim3(lr_grid(n)), dim3(256), 0, s, n, nullptr, SegView{}, 0, nullptr, r, nullptr, 0, L,
                       lda, rank, zv, w.tpart);
    return hipGetLastError();
}

hipError_t launch_lr_apply(int n, const double *r, const double *L, long lda, int rank, SegView zv, const LrWork &w,
                           const Scalars *sc, hipStream_t s)
{
    hipLaunchKernelGGL(k_lr_apply, dim3(lr_grid(n)), dim3(256), 0, s, n, r, L, lda, rank, w.C, w.head, w.tpart, lr_grid(n), sc, zv);
    return hipGetLastError();
}

}  // namespace cgx
