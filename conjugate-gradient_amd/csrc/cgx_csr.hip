// cgx_csr.hip -- K1 on CSR storage (CGX_MATRIX_CSR, opt-in), plan variant 7.
//
// Same contract as the banded K1 (k_spmv_dia, cgx_kernels.hip): the iteration head (or its Jacobi form), p_new = r + beta p_old
// formed on the fly and stored once, Ap of the shard's rows, one p.Ap partial per workgroup in partials[blockIdx.x], no
// atomics.  K3, the exchange of every transport and the host loop are shared unchanged.
//
// Layout: L consecutive lanes of a wave64 share one row (L = 1, 2, 4, ..., 64), so a wave covers 64 / L rows per pass and the
// workgroups stride over the row block.  Summation order, part of the contract: lane l of a row's group accumulates the
// entries start + l, start + l + L, ... in ascending order as one fma chain from +0.0; the L lane sums are combined by a
// fixed butterfly (group_sum, cgx_device.h).  A row's result therefore depends only on (row, L) -- not on the grid, the shard
// or the transport -- and with L = 1 the chain is the banded direct form's order (its zero entries add exactly nothing), so
// on the generated matrix Ap equals variant 30001 bit for bit.
//
// Values and columns are streamed once (non-temporal loads); the vectors are gathered through L2 and the Infinity Cache.
// A trip issues the column and value loads of CH entries, then the CH vector gathers, then the fmas.
//
// Load balance: a row is summed by one L-lane group, whatever its length.  Rows far longer than the mean therefore run
// imbalanced (the wave that holds one waits for it); a load-balanced form (row binning or merge-path) is the next step and
// not done here.
#include "cgx_kernels.h"
#include "cgx_device.h"

#include <hip/hip_ext.h>

#include <cmath>

namespace cgx {

namespace {

enum { kPlain = 0, kFusedSingle = 1, kFusedJacobi = 2 };

constexpr int csr_chunk(int L) { return L <= 2 ? 8 : 4; }   // entries in flight per lane and trip

template <int MODE, int L>
__global__ __launch_bounds__(256) void k_spmv_csr(CsrView cv, int rows, int row0, long lda, const double *__restrict__ v,
                                                   double *__restrict__ p_new, SegView sv, double *__restrict__ Ap,
                                                   double *__restrict__ partials, Scalars *sc, int k, double tol)
{
    constexpr bool FUSED = MODE != kPlain;
    constexpr bool PRE = MODE == kFusedJacobi;   // sv is z, not r: p = z + beta p_old
    constexpr int CH = csr_chunk(L);
    constexpr int G = 64 / L;                    // rows per wave and pass
    __shared__ double lds[4];
    const double *rfull = sv.base;               // FUSED: the replicated r (or z), zero padded up to lda
    double beta = 0.0;
    if constexpr (FUSED) {
        int done;
        const IterHead h = iteration_head_t<PRE>(sc, sv, k, tol, &done);
        if (done || h.stop) return;
        beta = h.beta;
        // p_new for the columns that are not rows of this shard (other ranks' rows and the pad); own rows: the row loop
        const long before = row0, after = lda - ((long)row0 + rows);
        for (long c = (long)blockIdx.x * 256 + threadIdx.x; c < before + after; c += (long)gridDim.x * 256) {
            const long cc = c < before ? c : c - before + row0 + rows;
            p_new[cc] = fma(beta, v[cc], rfull[cc]);
        }
    }
    const int lane = threadIdx.x & 63, sub = lane & (L - 1);
    const long wave = ((long)blockIdx.x * 256 + threadIdx.x) >> 6, nwaves = (long)gridDim.x * 4;
    double d = 0.0;
    // rb is the wave's first row: the trip count is the same for all 64 lanes, so the butterfly below runs on a full wave
    for (long rb = wave * G; rb < rows; rb += nwaves * G) {
        const long i = rb + lane / L;
        const bool valid = i < rows;
        const long ic = valid ? i : rows - 1;
        const long long start = cv.row_ptr[ic], end = valid ? cv.row_ptr[ic + 1] : start;
        double acc = 0.0;
        for (long long e0 = start + sub; e0 < end; e0 += (long long)CH * L) {
            int c[CH];
            double a[CH], q[CH], r[CH];
#pragma unroll
            for (int u = 0; u < CH; ++u) {
                const long long e = e0 + (long long)u * L;
                const long long ec = e < end ? e : end - 1;   // past the row's end: re-load the last entry, not used
                c[u] = __builtin_nontemporal_load(cv.col + ec);
                a[u] = __builtin_nontemporal_load(cv.vals + ec);
            }
#pragma unroll
            for (int u = 0; u < CH; ++u) {
                q[u] = v[c[u]];
                if constexpr (FUSED) r[u] = rfull[c[u]];
            }
#pragma unroll
            for (int u = 0; u < CH; ++u) {
                if (e0 + (long long)u * L < end) {
                    double qj = q[u];
                    if constexpr (FUSED) qj = fma(beta, qj, r[u]);             // same bits as the stored p_new[j]
                    acc = fma(a[u], qj, acc);                                  // cg.cc:100-102
                }
            }
        }
        acc = group_sum<L>(acc);
        if (valid && sub == 0) {
            const long g = row0 + i;
            double pg = v[g];
            if constexpr (FUSED) {
                pg = fma(beta, pg, rfull[g]);
                p_new[g] = pg;
            }
            Ap[i] = acc;
            d = fma(pg, acc, d);                                               // cg.cc:105
        }
    }
    d = block_sum<4>(d, lds);
    if (threadIdx.x == 0) partials[blockIdx.x] = d;
}

// generate_lap2d_matrix (cg.cc:159-188) into CSR, one thread per row.  Row g holds 1 + [g > 0] + [g < size-1] + [g > inc] +
// [g < size-1-inc] non-zeros (inc >= 1: the five columns are distinct), so its first entry is lap2d_prefix(g) - lap2d_prefix(row0).
__host__ __device__ inline long long lap2d_prefix(long long size, long long inc, long long g)
{
    auto atleast = [&](long long a) { return g > a ? g - a : 0; };                         // #{0 <= i < g : i >= a}
    auto atmost = [&](long long b) { return b < 0 ? 0 : (g < b + 1 ? g : b + 1); };       // #{0 <= i < g : i <= b}
    return g + atleast(1) + atmost(size - 2) + atleast(inc + 1) + atmost(size - 2 - inc);
}

__global__ __launch_bounds__(256) void k_csr_generate_lap2d(long long *__restrict__ row_ptr, int *__restrict__ col,
                                                             double *__restrict__ vals, int size, int row0, int rows, int inc)
{
    const long long base = lap2d_prefix(size, inc, row0);
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < rows; i += (long)gridDim.x * 256) {
        const long g = row0 + i;
        long long e = lap2d_prefix(size, inc, g) - base;
        if (i == 0) row_ptr[0] = 0;
        const long cand[5] = {g - 1 - inc, g - 1, g, g + 1, g + 1 + inc};   // ascending
#pragma unroll
        for (int t = 0; t < 5; ++t) {
            const long j = cand[t];
            if (j < 0 || j >= size) continue;
            const double a = lap2d_entry(size, inc, g, j);
            if (a == 0.0) continue;
            col[e] = (int)j;
            vals[e] = a;
            ++e;
        }
        row_ptr[i + 1] = e;
    }
}

__global__ __launch_bounds__(256) void k_csr_diag_slice(CsrView cv, int rows, int row0, double *__restrict__ dst)
{
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < rows; i += (long)gridDim.x * 256) {
        const int g = row0 + (int)i;
        long long lo = cv.row_ptr[i], hi = cv.row_ptr[i + 1];   // columns ascending: binary search for g
        while (lo < hi) {
            const long long mid = lo + (hi - lo) / 2;
            if (cv.col[mid] < g) lo = mid + 1;
            else hi = mid;
        }
        dst[i] = (lo < cv.row_ptr[i + 1] && cv.col[lo] == g) ? cv.vals[lo] : 0.0;
    }
}

// Block-Jacobi set-up: k_bj_col_slice on CSR storage -- the entry (row0 + i, s(row0 + i) + t) found as
// k_csr_diag_slice finds the diagonal, 0 where the row stores none or the column lies past n.
__global__ __launch_bounds__(256) void k_csr_bj_col_slice(CsrView cv, int n, int rows, int row0, int block, int t0,
                                                           double *__restrict__ dst, long dst_stride)
{
    const int t = t0 + (int)blockIdx.y;
    double *d = dst + (long)blockIdx.y * dst_stride;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < rows; i += (long)gridDim.x * 256) {
        const long g = row0 + i;
        const long c = g - g % block + t;
        long long lo = cv.row_ptr[i], hi = cv.row_ptr[i + 1];
        while (lo < hi) {
            const long long mid = lo + (hi - lo) / 2;
            if (cv.col[mid] < c) lo = mid + 1;
            else hi = mid;
        }
        d[i] = (c < n && lo < cv.row_ptr[i + 1] && cv.col[lo] == c) ? cv.vals[lo] : 0.0;
    }
}

struct CsrArgs {
    CsrView cv;
    int rows, row0;
    long lda;
    const double *v;
    double *p_new;
    SegView sv;
    double *Ap, *partials;
    Scalars *sc;
    int k;
    double tol;
    hipEvent_t e0, e1;
};

template <int MODE, int L>
hipError_t launch_csr_l(const GemvPlan &pl, const CsrArgs &g, hipStream_t s)
{
    hipExtLaunchKernelGGL((k_spmv_csr<MODE, L>), dim3(pl.grid), dim3(256), 0, s, g.e0, g.e1, 0, g.cv, g.rows, g.row0, g.lda, g.v,
                          g.p_new, g.sv, g.Ap, g.partials, g.sc, g.k, g.tol);
    return hipGetLastError();
}

template <int MODE>
hipError_t dispatch_csr(const GemvPlan &pl, const CsrArgs &g, hipStream_t s)
{
    switch (pl.R) {
    case 1: return launch_csr_l<MODE, 1>(pl, g, s);
    case 2: return launch_csr_l<MODE, 2>(pl, g, s);
    case 4: return launch_csr_l<MODE, 4>(pl, g, s);
    case 8: return launch_csr_l<MODE, 8>(pl, g, s);
    case 16: return launch_csr_l<MODE, 16>(pl, g, s);
    case 32: return launch_csr_l<MODE, 32>(pl, g, s);
    case 64: return launch_csr_l<MODE, 64>(pl, g, s);
    default: return hipErrorInvalidValue;
    }
}

int capped_grid(long total, int cap)
{
    const long g = (total + 255) / 256;
    return (int)(g < 1 ? 1 : (g < cap ? g : cap));
}

}  // namespace

bool csr_variant_ok(int variant)
{
    if (variant <= 0) return true;
    const int L = variant - kCsrVariantBase;
    return L >= 1 && L <= 64 && (L & (L - 1)) == 0;
}

GemvPlan plan_csr(int rows, long long nnz, int variant)
{
    GemvPlan pl{};
    pl.variant = 7;
    pl.split = 1;
    pl.waves = 4;
    pl.nt = 1;
    // the grid depends on rows only: 64 rows per workgroup pass, at most 2048 workgroups (K3 folds at most 2048 partials per
    // rank, as for plan_dia); above that the workgroups stride
    pl.grid = rows > 0 ? (rows + 63) / 64 : 1;
    if (pl.grid > 2048) pl.grid = 2048;
    int L;
    if (variant > kCsrVariantBase) {
        L = variant - kCsrVariantBase;
    } else {
        // Default lanes per row from the shard's mean entries per row: the smallest power of two L with 8 L >= mean, at most 64.
        // From the sweep of tools/csr_bench.py (profiles/csr/): at 5 entries per row L = 1 is the fastest
        // (774 us at 2^24 rows against 858 for L = 4 and 1549 for L = 8); at 38 per row (the skewed matrix) L = 8 ... 32 lie
        // within 2.5 % of each other and L = 1 is 2.3x slower.
        const double mean = rows > 0 ? (double)nnz / rows : 0.0;
        L = 1;
        while (L < 64 && 8.0 * L < mean) L *= 2;
    }
    pl.R = L;
    pl.U = csr_chunk(L);
    pl.rows_per_wg = 256 / L;
    return pl;
}

hipError_t launch_spmv_csr_plain(const GemvPlan &pl, const CsrView &cv, int rows, int row0, long lda, const double *v_full,
                                 double *Ap, double *partials, hipStream_t s)
{
    return dispatch_csr<kPlain>(pl, CsrArgs{cv, rows, row0, lda, v_full, nullptr, SegView{}, Ap, partials, nullptr, 0, 0.0,
                                            nullptr, nullptr}, s);
}

hipError_t launch_spmv_csr_fused(const GemvPlan &pl, const CsrView &cv, int rows, int row0, long lda, const double *p_old,
                                 double *p_new, SegView seg, double *Ap, double *partials, Scalars *sc, int k, double tol,
                                 hipStream_t s, hipEvent_t e_start, hipEvent_t e_stop, bool jacobi)
{
    const CsrArgs g{cv, rows, row0, lda, p_old, p_new, seg, Ap, partials, sc, k, tol, e_start, e_stop};
    return jacobi ? dispatch_csr<kFusedJacobi>(pl, g, s) : dispatch_csr<kFusedSingle>(pl, g, s);
}

long long lap2d_csr_nnz(int size, int row0, int rows)
{
    const int inc = (int)floor(sqrt((double)size));   // cg.cc:175
    return lap2d_prefix(size, inc, (long long)row0 + rows) - lap2d_prefix(size, inc, row0);
}

hipError_t launch_csr_generate_lap2d(long long *row_ptr, int *col, double *vals, int size, int row0, int rows, hipStream_t s)
{
    if (rows <= 0) return hipSuccess;
    const int inc = (int)floor(sqrt((double)size));   // cg.cc:175
    hipLaunchKernelGGL(k_csr_generate_lap2d, dim3(capped_grid(rows, 8192)), dim3(256), 0, s, row_ptr, col, vals, size, row0, rows, inc);
    return hipGetLastError();
}

hipError_t launch_csr_diag_slice(const CsrView &cv, int rows, int row0, double *dst, hipStream_t s)
{
    if (rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_csr_diag_slice, dim3(capped_grid(rows, 1024)), dim3(256), 0, s, cv, rows, row0, dst);
    return hipGetLastError();
}

hipError_t launch_csr_bj_col_slice(const CsrView &cv, int n, int rows, int row0, int block, int t0, int nt, double *dst,
                                   long dst_stride, hipStream_t s)
{
    if (rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_csr_bj_col_slice, dim3(capped_grid(rows, 1024), nt), dim3(256), 0, s, cv, n, rows, row0, block, t0, dst,
                       dst_stride);
    return hipGetLastError();
}

}  // namespace cgx
