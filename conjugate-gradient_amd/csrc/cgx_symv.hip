// cgx_symv.hip -- K1 for a symmetric A on one GPU (plan variant 6): A p from the upper triangle alone.
//
// CG needs A = A^T (cg.cc runs on generate_lap2d_matrix's output and on symmetric Matrix-Market files), so every off-diagonal
// tile A_IJ (I < J) of the upper triangle serves twice: A_IJ p_J goes into the rows of block I and A_IJ^T p_I into the rows of
// block J.  The lower triangle is never read: the bytes K1 streams per iteration fall from 8 n^2 to 8 n^2 (nb + 1) / (2 nb)
// (nb = blocks of B rows).  Whether A is exactly symmetric is decided by k_symmetric_check when the matrix is written
// (cgx_context.cpp, plan_symmetric); the plan follows that flag, nothing else.
//
// One iteration is then three kernels:
//   k_symv_tiles  the iteration head of K1 (r.r fold, break test, beta), p_new = r + beta p_old formed on the fly and stored once
//                 (by the diagonal tile of its block), and for every tile (I, J), I <= J, of the upper triangle:
//                    slot J of block I  <- A_IJ p_J        (row piece; a diagonal tile is read whole and gives this one only)
//                    slot I of block J  <- A_IJ^T p_I      (column piece, I < J)
//                 so every block has exactly nb slots, each written once: parts = nb x lda doubles, slot s of row i at
//                 parts[s * lda + i]
//   k_symv_fold   Ap[i] = the nb slots of row i added in one fixed order; one p.Ap partial per workgroup into the segment tail
//   K3            unchanged (cgx_kernels.hip), it folds the fold's partials instead of K1's
// No floating-point atomics; every sum has a fixed order, whichever workgroup handles a tile.
#include "cgx_kernels.h"
#include "cgx_device.h"

#include <hip/hip_ext.h>

namespace cgx {

// Tile t of the upper triangle in strip order -- (0,0) (0,1) ... (0,nb-1) (1,1) ... -- to (I, J).  Strip I starts at
// I nb - I (I - 1) / 2; the root of that quadratic gives I up to rounding, the two loops fix the rounding.
__device__ __forceinline__ long strip_start(long I, long nb) { return I * nb - I * (I - 1) / 2; }
__device__ __forceinline__ void tri_tile(long t, long nb, long *I, long *J)
{
    const double b = 2.0 * (double)nb + 1.0;
    long i = (long)((b - sqrt(b * b - 8.0 * (double)t)) * 0.5);
    i = i < 0 ? 0 : (i > nb - 1 ? nb - 1 : i);
    while (i + 1 < nb && strip_start(i + 1, nb) <= t) ++i;
    while (i > 0 && strip_start(i, nb) > t) --i;
    *I = i;
    *J = i + (t - strip_start(i, nb));
}

// One workgroup of 4 waves walks a run of consecutive tiles of the triangle (runs of the grid differ by one tile at most; along
// a strip the tiles are consecutive 2-KiB pieces of the same B rows).  Per tile, wave w takes B/4 rows in batches of R, every
// lane 16 B of each of H 1-KiB column pieces per row (16 loads of A in flight per lane, as K1's (8,2)):
//   - row piece: per-lane products, summed over the wave with wave_sum_rows (one shared reduction for R rows), into LDS;
//   - column piece: per-lane register accumulators (the lane owns its 2H columns over all of the wave's rows), p of the row
//     broadcast from the lane that holds it (v_readlane), the 4 waves combined in LDS in wave order.
// One barrier per tile; LDS is double buffered by tile parity, so the next tile's writes never meet this tile's reads.
// FUSED: the iteration head first (every wave, as K1: no barrier in front of it), p = r + beta p_old in registers.
// k_pcg_symv_tiles (Jacobi): the same body (cgx_symv_tiles.inc) with PRE = true -- sv is the replicated z
// instead of r, which vec2 / vec1 read through the same pointer, and the head is the PRECOND form (beta from r.z, the break from r.r).
template <int B, bool FUSED>
__global__ __launch_bounds__(256, 4) void k_symv_tiles(const double *__restrict__ A, long lda, int n, int ncols, int nb, long tiles,
                                                       const double *__restrict__ v, double *__restrict__ p_new, SegView sv,
                                                       double *__restrict__ parts, Scalars *sc, int k, double tol)
{
    constexpr bool PRE = false;
#include "cgx_symv_tiles.inc"
}

// The Jacobi form (fused only): sv is the replicated z; the PRECOND head
template <int B>
__global__ __launch_bounds__(256, 4) void k_pcg_symv_tiles(const double *__restrict__ A, long lda, int n, int ncols, int nb, long tiles,
                                                       const double *__restrict__ v, double *__restrict__ p_new, SegView sv,
                                                       double *__restrict__ parts, Scalars *sc, int k, double tol)
{
    constexpr bool FUSED = true;
    constexpr bool PRE = true;
#include "cgx_symv_tiles.inc"
}

// Ap[i] = the nb slots of row i, i < Sr; tail[wg] = the workgroup's part of p . Ap (cg.cc:105).  A workgroup owns 128 rows (a
// lane = a pair of rows, 16 B); its 8 waves split the slots in 8 consecutive runs, each added in ascending order, and the runs
// are added in wave order: one fixed order.  Rows from n on hold zeros in every slot (the buffer is zeroed when it is made and
// never written there), so Ap[n] of an odd n stays 0.  FUSED: nothing is stored once converged (a predicate on the stores, as
// in k_prefold_ap, so that the loads need not wait for the flag).
constexpr int kFoldWaves = 8;
constexpr int kFoldRows = 128;
template <bool FUSED>
__global__ __launch_bounds__(kFoldWaves * 64) void k_symv_fold(const double *__restrict__ parts, long lda, int nb, int Sr,
                                                               const double *__restrict__ p, double *__restrict__ Ap,
                                                               double *__restrict__ tail, const Scalars *sc)
{
    __shared__ d2 red[kFoldWaves][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int done = FUSED ? sc->done : 0;
    const int row = (int)blockIdx.x * kFoldRows + 2 * lane;
    const int rc = row < Sr ? row : 0;
    const int s0 = nb * w / kFoldWaves, s1 = nb * (w + 1) / kFoldWaves;
    d2 acc{0.0, 0.0};
    for (int s = s0; s < s1; s += 8) {
        d2 x[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {   // unconditional loads (clamped slot): all eight in flight together
            const int su = s + u < s1 ? s + u : s1 - 1;
            x[u] = *reinterpret_cast<const d2 *>(parts + (long)su * lda + rc);
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            acc.x = s + u < s1 ? acc.x + x[u].x : acc.x;
            acc.y = s + u < s1 ? acc.y + x[u].y : acc.y;
        }
    }
    d2 pv = *reinterpret_cast<const d2 *>(p + rc);
    red[w][lane] = acc;
    __syncthreads();
    if (w != 0) return;
    d2 a = red[0][lane];
#pragma unroll
    for (int i = 1; i < kFoldWaves; ++i) {
        a.x += red[i][lane].x;
        a.y += red[i][lane].y;
    }
    if (row >= Sr) { a = d2{0.0, 0.0}; pv = d2{0.0, 0.0}; }
    if (!done && row < Sr) *reinterpret_cast<d2 *>(Ap + row) = a;
    const double d = wave_sum(fma(pv.y, a.y, pv.x * a.x));
    if (!done && lane == 0) tail[blockIdx.x] = d;
}

// Is A (n x n at pitch lda) exactly symmetric?  Pairs of 32 x 32 tiles (I <= J): tile (J, I) goes into LDS transposed, tile (I, J)
// is compared with it element by element as 64-bit words (so +0 / -0 and NaN payloads count as differences).  Any mismatch raises
// *mismatch (an integer flag; set-up only).  Every element outside the diagonal tiles is read once; pad columns are not read.
__global__ __launch_bounds__(256) void k_symmetric_check(const double *__restrict__ A, long lda, int n, long nt, long pairs, int *mismatch)
{
    __shared__ unsigned long long tt[32][33];
    const int x = threadIdx.x & 31, y0 = threadIdx.x >> 5;
    const unsigned long long *Ab = reinterpret_cast<const unsigned long long *>(A);
    for (long q = blockIdx.x; q < pairs; q += gridDim.x) {
        long I, J;
        tri_tile(q, nt, &I, &J);
#pragma unroll
        for (int y = y0; y < 32; y += 8) {   // tt[x][y] = A(J*32 + y, I*32 + x)
            const long r = J * 32 + y, c = I * 32 + x;
            tt[x][y] = (r < n && c < n) ? Ab[r * lda + c] : 0ull;
        }
        __syncthreads();
        bool bad = false;
#pragma unroll
        for (int y = y0; y < 32; y += 8) {   // A(I*32 + y, J*32 + x) against tt[y][x] = A(J*32 + x, I*32 + y)
            const long r = I * 32 + y, c = J * 32 + x;
            if (r < n && c < n) bad |= Ab[r * lda + c] != tt[y][x];
        }
        if (bad) atomicOr(mismatch, 1);
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
GemvPlan plan_symv(int n, long lda, int cus, int run)
{
    GemvPlan pl{};
    pl.variant = 6;
    pl.R = kSymvTile;
    pl.waves = 4;
    pl.nt = 1;
    pl.split = (n + kSymvTile - 1) / kSymvTile;                      // nb: blocks = slots per block
    const long tiles = (long)pl.split * (pl.split + 1) / 2;
    // run = 0: 4 workgroups per CU (128 VGPRs, 20 KiB of LDS each), what is resident at once; run > 0: tiles / run workgroups,
    // which the dispatcher hands to the CUs as they come free ("variant 6")
    long slots = run > 0 ? tiles / run : 4L * (cus > 0 ? cus : 256);
    if (slots < 1) slots = 1;
    if (slots > (1L << 30)) slots = 1L << 30;
    pl.grid = (int)(tiles < slots ? tiles : slots);
    pl.U = (int)((tiles + pl.grid - 1) / pl.grid);                   // tiles of the longest run
    const int Sr = (n + 1) / 2 * 2;
    pl.light = (Sr + kFoldRows - 1) / kFoldRows;                     // fold workgroups = p.Ap partials
    pl.ncols = (n + 1) & ~1;
    if (pl.ncols > (int)lda) pl.ncols = (int)lda;
    pl.rows_per_wg = kSymvTile;
    return pl;
}

namespace {

template <bool FUSED, bool PRE = false>
hipError_t launch_symv(const GemvPlan &pl, const double *A, long lda, int n, const double *v, double *p_new, SegView sv,
                       double *parts, double *Ap, double *tail, Scalars *sc, int k, double tol, hipStream_t s, hipEvent_t e0,
                       hipEvent_t e1)
{
    if (pl.variant != 6 || pl.R != kSymvTile || n < 2) return hipErrorInvalidValue;
    const long tiles = (long)pl.split * (pl.split + 1) / 2;
    if constexpr (PRE)
        hipExtLaunchKernelGGL((k_pcg_symv_tiles<kSymvTile>), dim3(pl.grid), dim3(256), 0, s, e0, nullptr, 0, A, lda, n, pl.ncols,
                              pl.split, tiles, v, p_new, sv, parts, sc, k, tol);
    else
        hipExtLaunchKernelGGL((k_symv_tiles<kSymvTile, FUSED>), dim3(pl.grid), dim3(256), 0, s, e0, nullptr, 0, A, lda, n, pl.ncols,
                              pl.split, tiles, v, p_new, sv, parts, sc, k, tol);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const int Sr = (n + 1) / 2 * 2;
    hipExtLaunchKernelGGL((k_symv_fold<FUSED>), dim3(pl.light), dim3(kFoldWaves * 64), 0, s, nullptr, e1, 0, parts, lda, pl.split, Sr,
                          FUSED ? p_new : v, Ap, tail, sc);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_symv_plain(const GemvPlan &pl, const double *A, long lda, int n, const double *v, double *parts, double *Ap,
                             double *partials, hipStream_t s)
{
    return launch_symv<false>(pl, A, lda, n, v, nullptr, SegView{}, parts, Ap, partials, nullptr, 0, 0.0, s, nullptr, nullptr);
}

hipError_t launch_symv_fused(const GemvPlan &pl, const double *A, long lda, int n, const double *p_old, double *p_new, SegView seg,
                             double *parts, double *Ap, double *partials, Scalars *sc, int k, double tol, hipStream_t s,
                             hipEvent_t e_start, hipEvent_t e_stop, bool jacobi)
{
    if (jacobi) return launch_symv<true, true>(pl, A, lda, n, p_old, p_new, seg, parts, Ap, partials, sc, k, tol, s, e_start, e_stop);
    return launch_symv<true>(pl, A, lda, n, p_old, p_new, seg, parts, Ap, partials, sc, k, tol, s, e_start, e_stop);
}

hipError_t launch_symmetric_check(const double *A, long lda, int n, int *mismatch, hipStream_t s)
{
    const long nt = ((long)n + 31) / 32, pairs = nt * (nt + 1) / 2;
    const long grid = pairs < 8192 ? pairs : 8192;
    hipLaunchKernelGGL(k_symmetric_check, dim3((unsigned)grid), dim3(256), 0, s, A, lda, n, nt, pairs, mismatch);
    return hipGetLastError();
}

}  // namespace cgx
