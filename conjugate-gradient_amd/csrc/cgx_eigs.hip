// cgx_eigs.hip -- the kernels of cgx_eigenpairs: Lanczos with full reorthogonalisation (classical Gram-Schmidt
// against the whole kept basis, run twice per step), the Ritz-vector combine and the residual norms.
//
// The basis is ONE vector per slot: element i of q_s is at Q[s * lda + i], (steps + 1) * lda doubles in all -- more than 2^31 at large
// n, hence size_t offsets throughout.  Step t behind the plain multi-vector K1 at width 1 (y = A q_t and the partials of q_t . y):
//
//   k_eigs_project<true>    alpha_t folded from K1m's partials; w = y - alpha_t q_t - beta_(t-1) q_(t-1) made in registers (chunk 0
//                           stores it); the partials of h = Q_t^T w, one per (slot, 256-row tile)
//   k_eigs_subtract<false>  h folded per slot in ascending tile order (every workgroup: the same h), w -= Q_t h
//   k_eigs_project<false>   the partials of h' = Q_t^T w
//   k_eigs_subtract<true>   w -= Q_t h', and one ||w||^2 partial per tile
//   k_eigs_normalise        beta_t = ||w||, the breakdown test, q_(t+1) = w / beta_t stored straight into slot t + 1
//
// The projection runs on a grid of row tiles x slot chunks (kEigsChunk slots each): a wave keeps its 256 elements of w in registers
// (four per lane), streams 8 slots against them and reduces the 8 sums together (wave_sum_rows<8>).  The subtraction is the access
// pattern of k_funm_combine: a thread owns one element and walks the slots in ascending order, ONE fma chain from +0.0; the loads of
// kUnroll slots are issued ahead of their fmas.  Both read the basis with non-temporal 8-byte loads (correct at any row pitch), so a
// pass reads it exactly twice.  Slots behind t and the pad rows of a slot are never read; the kernels that write a vector K1m will
// read (k_eigs_init, k_eigs_normalise, k_eigs_combine) also write the zero K1m's 16-byte pieces reach behind an odd n.
//
// Every workgroup folds the same partials in the same fixed order and so takes the same decision; workgroup 0 alone writes the
// scalars and histories, with plain stores.  No grid, tile or sum order depends on the number of steps of the call: a longer run has
// the shorter one's alpha, beta and q as a bitwise prefix.  No floating-point atomics, no scratch.
#include "cgx_kernels.h"
#include "cgx_device.h"

namespace cgx {

namespace {

constexpr double kEigsBreak = 0x1.0p-36;   // beta_t <= 2^-36 max |alpha|: an invariant subspace (as cgx_lanczos)
constexpr int kUnroll = 16;                 // slots in flight per thread of the subtraction
constexpr int kFoldUnroll = 16;             // tiles in flight per thread of its fold of h
constexpr int kCombineThreads = 64;         // one wave per workgroup: n / 64 workgroups reach every CU from n = 16384 on
constexpr int kWaveSlots = kEigsChunk / 4;   // slots per wave of a projection workgroup

// One workgroup: ||v0||^2 in a fixed order, q_0 = v0 / ||v0|| in place, the scalars reset; a zero or non-finite v0 is marked bad and
// no step runs.
__global__ __launch_bounds__(1024) void k_eigs_init(int n, double *__restrict__ q0, EigsScalars *sc)
{
    __shared__ double lds[16];
    double s = 0.0;
    for (long i = threadIdx.x; i < n; i += 1024) {
        const double v = q0[i];
        s = fma(v, v, s);
    }
    s = wave_sum(s);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) lds[wv] = s;
    __syncthreads();
    double tot = lds[0];
    for (int u = 1; u < 16; ++u) tot += lds[u];
    const bool ok = tot > 0.0 && tot <= 1.7976931348623157e308;   // false for 0, inf and NaN
    if (threadIdx.x == 0) {
        sc->amax[0] = 0.0;
        sc->amax[1] = 0.0;
        sc->z2 = tot;
        sc->m = ok ? kEigsLive : -1;
        sc->bad = ok ? 0 : 1;
    }
    if (!ok) return;
    const double nrm = sqrt(tot);
    const long ncols = ((long)n + 1) & ~1L;
    for (long i = threadIdx.x; i < ncols; i += 1024) q0[i] = i < n ? q0[i] / nrm : 0.0;
}

// Workgroup (b, c) = rows [256 b, 256 b + 256) against slots [kEigsChunk c, kEigsChunk c + kEigsChunk), clipped to 0 .. t.
template <bool FIRST>
__global__ __launch_bounds__(256) void k_eigs_project(int n, long lda, int t, const double *__restrict__ Q, const double *__restrict__ Y,
                                                      double *__restrict__ W, const double *__restrict__ k1p, int g1,
                                                      double *__restrict__ hp, double *__restrict__ ha, const double *__restrict__ hb,
                                                      EigsScalars *sc)
{
    __shared__ double lds[4];
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int mrun = sc->m;
    double alpha = 0.0, beta = 0.0, amax = 0.0;
    if constexpr (FIRST) {
        const double cs = fold_pap(k1p, 1, 0, g1);
        amax = sc->amax[t & 1];
        if (t > 0) beta = hb[t - 1];
        if (mrun <= t) return;                             // frozen in an earlier step, or a bad start vector (uniform)
        alpha = block_sum<4>(cs, lds);                     // alpha_t = q_t . A q_t
        if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
            ha[t] = alpha;
            const double aa = fabs(alpha);
            sc->amax[(t + 1) & 1] = aa > amax ? aa : amax;
        }
    } else {
        if (mrun <= t) return;
    }
    const long row0 = (long)blockIdx.x * kEigsTile + lane;
    double w[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const long i = row0 + 64 * k;
        const long ic = i < n ? i : n - 1;
        double v;
        if constexpr (FIRST) {
            const double y = Y[ic], q = Q[(size_t)t * (size_t)lda + (size_t)ic];
            const double u = t > 0 ? Q[(size_t)(t - 1) * (size_t)lda + (size_t)ic] : 0.0;
            v = fma(-beta, u, fma(-alpha, q, y));
            if (blockIdx.y == 0 && wv == 0 && i < n) W[i] = v;
        } else {
            v = W[ic];
        }
        w[k] = i < n ? v : 0.0;
    }
    const int s0 = (int)blockIdx.y * kEigsChunk + wv * kWaveSlots;
    if (s0 > t) return;                                    // (no barrier follows)
    double qv[kWaveSlots][4];
#pragma unroll
    for (int u = 0; u < kWaveSlots; ++u) {
        const int s = s0 + u <= t ? s0 + u : t;            // clamped, the sum is dropped below: slots behind t are never read
        const double *q = Q + (size_t)s * (size_t)lda;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const long i = row0 + 64 * k;
            qv[u][k] = __builtin_nontemporal_load(q + (size_t)(i < n ? i : n - 1));
        }
    }
    double acc[kWaveSlots];
#pragma unroll
    for (int u = 0; u < kWaveSlots; ++u) {
        acc[u] = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[u] = fma(w[k], row0 + 64 * k < n ? qv[u][k] : 0.0, acc[u]);
    }
    const int u = wave_sum_rows<kWaveSlots>(acc, lane);   // the slot (of the wave's) whose total this lane holds
    if ((lane & (64 / kWaveSlots - 1)) == 0 && s0 + u <= t) hp[(size_t)blockIdx.x * kEigsSlotPitch + (size_t)(s0 + u)] = acc[0];
}

// Workgroup b = rows [256 b, 256 b + 256).  SECOND: the pass behind which the step is normalised.
template <bool SECOND>
__global__ __launch_bounds__(256) void k_eigs_subtract(int n, long lda, int t, const double *__restrict__ Q, double *__restrict__ W,
                                                       const double *__restrict__ hp, int tiles, double *__restrict__ h_out,
                                                       double *__restrict__ wwp, const EigsScalars *sc)
{
    __shared__ double h[kEigsSlotPitch];
    __shared__ double lds[4];
    if (sc->m <= t) return;
    for (int s = threadIdx.x; s <= t; s += 256) {
        const double *p = hp + s;
        double a = 0.0;                                    // ascending tiles: the same in every workgroup
        int b = 0;
        for (; b + kFoldUnroll <= tiles; b += kFoldUnroll) {   // the loads of kFoldUnroll tiles ahead of their additions
            double v[kFoldUnroll];
#pragma unroll
            for (int u = 0; u < kFoldUnroll; ++u) v[u] = p[(size_t)(b + u) * kEigsSlotPitch];
#pragma unroll
            for (int u = 0; u < kFoldUnroll; ++u) a += v[u];
        }
        for (; b < tiles; ++b) a += p[(size_t)b * kEigsSlotPitch];
        h[s] = a;
        if (blockIdx.x == 0) h_out[s] = a;
    }
    __syncthreads();
    const long i = (long)blockIdx.x * kEigsTile + threadIdx.x;
    const bool in = i < n;
    const double *q = Q + (size_t)(in ? i : n - 1);
    const size_t stride = (size_t)lda;
    double acc = 0.0;
    int s = 0;
    for (; s + kUnroll <= t + 1; s += kUnroll) {
        double v[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) v[u] = __builtin_nontemporal_load(q + (size_t)(s + u) * stride);
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) acc = fma(h[s + u], v[u], acc);
    }
    for (; s <= t; ++s) acc = fma(h[s], __builtin_nontemporal_load(q + (size_t)s * stride), acc);
    double wn = 0.0;
    if (in) {
        wn = W[i] - acc;
        W[i] = wn;
    }
    if constexpr (SECOND) {
        const double ww = block_sum<4>(wn * wn, lds);
        if (threadIdx.x == 0) wwp[blockIdx.x] = ww;
    }
}

// Workgroup b = rows [256 b, 256 b + 256): beta_t, the breakdown test, q_(t+1) = w / beta_t.
__global__ __launch_bounds__(256) void k_eigs_normalise(int n, long lda, int t, double *__restrict__ Q, const double *__restrict__ W,
                                                        const double *__restrict__ wwp, int tiles, double *__restrict__ hb,
                                                        EigsScalars *sc)
{
    __shared__ double lds[4];
    const int mrun = sc->m;
    const double amax = sc->amax[(t + 1) & 1];             // max |alpha_s| over s <= t
    const double ws = fold_pap(wwp, 1, 0, tiles);
    if (mrun <= t) return;
    const double beta = sqrt(block_sum<4>(ws, lds));
    const bool writer = blockIdx.x == 0 && threadIdx.x == 0;
    if (writer) hb[t] = beta;
    if (beta <= kEigsBreak * amax) {                       // the space is invariant: the run is frozen with m = t + 1
        if (writer) sc->m = t + 1;
        return;
    }
    const long i = (long)blockIdx.x * kEigsTile + threadIdx.x;
    const long ncols = ((long)n + 1) & ~1L;
    if (i < ncols) Q[(size_t)(t + 1) * (size_t)lda + (size_t)i] = i < n ? W[i] / beta : 0.0;
}

// X_j[i] = sum over t < m of C[t * WD + j] q_t[i] for the WD vectors at once: q_t[i] is read ONCE and serves every accumulator; per
// element and vector one fma chain in ascending t from +0.0.  The coefficients are the same for the whole workgroup (scalar loads of
// the WD consecutive doubles of step t).  Vectors at j >= nev have zero coefficients and are not stored.
template <int WD>
__global__ __launch_bounds__(kCombineThreads) void k_eigs_combine(int n, long lda, int m, int nev, const double *__restrict__ Q,
                                                      const double *__restrict__ C, double *__restrict__ X, long ldx)
{
    constexpr int U = WD <= 4 ? 16 : 8;
    const long i = (long)blockIdx.x * kCombineThreads + threadIdx.x;
    const long ncols = ((long)n + 1) & ~1L;
    if (i >= ncols) return;
    const double *q = Q + (size_t)(i < n ? i : n - 1);
    const size_t stride = (size_t)lda;
    double acc[WD];
#pragma unroll
    for (int j = 0; j < WD; ++j) acc[j] = 0.0;
    int t = 0;
    for (; t + U <= m; t += U) {
        double v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) v[u] = __builtin_nontemporal_load(q + (size_t)(t + u) * stride);
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int j = 0; j < WD; ++j) acc[j] = fma(C[(size_t)(t + u) * WD + j], v[u], acc[j]);
    }
    for (; t < m; ++t) {
        const double v = __builtin_nontemporal_load(q + (size_t)t * stride);
#pragma unroll
        for (int j = 0; j < WD; ++j) acc[j] = fma(C[(size_t)t * WD + j], v, acc[j]);
    }
#pragma unroll
    for (int j = 0; j < WD; ++j)
        if (j < nev) X[(size_t)j * (size_t)ldx + (size_t)i] = i < n ? acc[j] : 0.0;
}

// One workgroup per vector: out[j] = || Y_j - theta_j X_j ||^2 in a fixed order (the shape of k_column_norms, cgx_multi.hip).
__global__ __launch_bounds__(1024) void k_eigs_residual(int n, long lda, const double *__restrict__ Y, const double *__restrict__ X,
                                                        const double *__restrict__ theta, double *__restrict__ out)
{
    __shared__ double lds[16];
    const int j = blockIdx.x;
    const double th = theta[j];
    double e = 0.0;
    for (long i = threadIdx.x; i < n; i += 1024) {
        const size_t off = (size_t)j * (size_t)lda + (size_t)i;
        const double d = fma(-th, X[off], Y[off]);
        e = fma(d, d, e);
    }
    e = wave_sum(e);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) lds[w] = e;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = lds[0];
        for (int u = 1; u < 16; ++u) s += lds[u];
        out[j] = s;
    }
}

bool step_args_ok(const EigsArgs &a)
{
    return a.n >= 1 && a.lda >= a.n && a.t >= 0 && a.t < kMaxLanczosSteps;
}

}  // namespace

int eigs_tiles(int n) { return (n + kEigsTile - 1) / kEigsTile; }

hipError_t launch_eigs_init(int n, double *q0, EigsScalars *sc, hipStream_t s)
{
    if (n < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_eigs_init, dim3(1), dim3(1024), 0, s, n, q0, sc);
    return hipGetLastError();
}

hipError_t launch_eigs_project(const EigsArgs &a, bool first, hipStream_t s)
{
    if (!step_args_ok(a)) return hipErrorInvalidValue;
    const dim3 grid(eigs_tiles(a.n), a.t / kEigsChunk + 1);
    if (first)
        hipLaunchKernelGGL(k_eigs_project<true>, grid, dim3(256), 0, s, a.n, a.lda, a.t, a.Q, a.Y, a.W, a.k1p, a.g1, a.hp, a.alpha, a.beta,
                           a.sc);
    else
        hipLaunchKernelGGL(k_eigs_project<false>, grid, dim3(256), 0, s, a.n, a.lda, a.t, a.Q, a.Y, a.W, a.k1p, a.g1, a.hp, a.alpha, a.beta,
                           a.sc);
    return hipGetLastError();
}

hipError_t launch_eigs_subtract(const EigsArgs &a, bool second, hipStream_t s)
{
    if (!step_args_ok(a)) return hipErrorInvalidValue;
    const int tiles = eigs_tiles(a.n);
    if (second)
        hipLaunchKernelGGL(k_eigs_subtract<true>, dim3(tiles), dim3(256), 0, s, a.n, a.lda, a.t, a.Q, a.W, a.hp, tiles, a.h, a.wwp, a.sc);
    else
        hipLaunchKernelGGL(k_eigs_subtract<false>, dim3(tiles), dim3(256), 0, s, a.n, a.lda, a.t, a.Q, a.W, a.hp, tiles, a.h, a.wwp, a.sc);
    return hipGetLastError();
}

hipError_t launch_eigs_normalise(const EigsArgs &a, hipStream_t s)
{
    if (!step_args_ok(a)) return hipErrorInvalidValue;
    const int tiles = eigs_tiles(a.n);
    hipLaunchKernelGGL(k_eigs_normalise, dim3(tiles), dim3(256), 0, s, a.n, a.lda, a.t, a.Q, a.W, a.wwp, tiles, a.beta, a.sc);
    return hipGetLastError();
}

hipError_t launch_eigs_combine(int n, long lda, int m, int nev, const double *Q, const double *C, double *X, long ldx, hipStream_t s)
{
    if (n < 1 || lda < n || ldx < n || m < 1 || m > kMaxLanczosSteps || nev < 1 || nev > kMaxEigenpairs) return hipErrorInvalidValue;
    const dim3 grid((n + kCombineThreads) / kCombineThreads), block(kCombineThreads);   // rows 0 .. n: the zero behind an odd n
    for_multi_width(nev, [&](auto w) { hipLaunchKernelGGL(k_eigs_combine<decltype(w)::value>, grid, block, 0, s, n, lda, m, nev, Q, C, X, ldx); });
    return hipGetLastError();
}

hipError_t launch_eigs_residual(int n, long lda, int nev, const double *Y, const double *X, const double *theta, double *out,
                                hipStream_t s)
{
    if (n < 1 || nev < 1 || nev > kMaxEigenpairs) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_eigs_residual, dim3(nev), dim3(1024), 0, s, n, lda, Y, X, theta, out);
    return hipGetLastError();
}

}  // namespace cgx
