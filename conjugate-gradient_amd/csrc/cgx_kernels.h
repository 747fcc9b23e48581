// cgx_kernels.h -- launch interface of the CDNA4 (gfx950) kernels of the CG hot path.
// The host code (cgx_context / cgx_matrix / cgx_solve / cgx_probe .cpp) sees only these plain functions; all device code is in the .hip files.
#pragma once

#include <hip/hip_runtime.h>

#include <type_traits>

namespace cgx {

// Small scalar exchange of the verification phase (cg.cc:144-151): every shard publishes kSlots doubles, the
// host sums slot v over ranks in rank order.
constexpr int kSlots = 4;
constexpr int kSlotConj = 0;   // ||Ax-b||^2 partial (also: p.Ap of the gemv probe)
constexpr int kSlotRr = 1;     // ||b||^2 partial
constexpr int kSlotX = 2;      // ||x||^2 partial
constexpr int kMaxRanks = 64;  // gathered[] holds kMaxRanks*kSlots doubles

// Device-resident scalar block of one shard.  Nothing in the iteration loop is read back by the
// host except `done` (polled every check_every iterations).
struct Scalars {
    double rs[2];          // rsold / rsnew ping-pong: rs[k&1] is rsold of iteration k          (cg.cc:91,116,132)
                           // (Jacobi: rho = r.z, the numerator of alpha and beta)
    double rr[2];          // Jacobi only: r.r in the same ping-pong, what the stopping test and the report use
    double local[kSlots];  // send buffer of the small scalar all-gather (verification phase)
    double dbg[4];
    int    done;           // set when sqrt(rsnew) < tol (cg.cc:120-121); later kernels exit at once
    int    k_final;        // k of the converging iteration
    unsigned pad[2];
};

// Segmented vector: P equal segments of S doubles, segment q = [ slice of rank q (Sr doubles, zero padded) |
// tail ].  Used for the exchanged Ap ([Ap slice | p.Ap partials], one in-place all-gather per iteration in
// place of MPI_Allreduce cg.cc:106 + MPI_Allgatherv cg.cc:135-136) and, with nranks = 1, for the replicated
// r ([r (lda) | r.r partials of K3's workgroups]).
struct SegView {
    double *base;     // this shard's copy of all P segments
    int S, Sr;        // segment stride, r part
    int n_loc;        // floor(n / nranks): rows of every rank but the last (cg.cc:255)
    int nranks;
    int n;
    int rank;         // this shard
    int seg_gap;      // S - n_loc: r[c] of owner q sits at base[c + q*seg_gap]
    unsigned div_magic, div_shift;   // c / n_loc == umulhi(c, div_magic) >> div_shift for 0 <= c < 2^31
};

// Fill seg_gap and the division magic of a SegView whose S, n_loc, nranks are set.
void seg_finalize(SegView *sv);

struct GemvPlan {
    int variant;     // 1 = column-split (p from L2 to registers), 2 = row-split (p tiles staged in LDS),
                     // 3 = banded storage (DiaView), one thread per row; 7 = CSR storage (CsrView), R lanes per row
    int R;           // rows per wave (variant 2) or per workgroup (variant 1)
    int U;           // column-step unroll
    int waves;       // waves per workgroup
    int nt;          // non-temporal loads of A
    int grid;        // workgroups
    int rows_per_wg;
    int ncols;       // columns the sweep covers: the logical n rounded up to even (16-B pieces); the pad columns up to the
                     // pitch are zero in A and in every vector and are never touched
    int split;       // variant 1, fused launches only: column pieces per row group (1 = none).  grid counts ALL workgroups
                     // (row groups x split) = the number of p.Ap partials; a plain launch uses grid / split
    int light;       // variant 1: the one-round form (first trip issued ahead of the iteration head, 256 registers to spend;
                     // see k_gemv_colsplit); variant 3: the LDS-window form of K1b
};

// Choose the K1 shape for a shard of `rows` x `n` held at pitch `lda` (variant 0 = default).  allow_split: the consumer of
// Ap adds column pieces itself (every multi-rank transport: launch_prefold_ap or the fused P2P update), so the default may
// cut the columns of a row group into pieces.
GemvPlan plan_gemv(int variant, int rows, int n, long lda, bool allow_split = false);

// K1, plain form: Ap = A[rows x lda] * v ; partials[wg] = sum over the workgroup's rows of v_local[i]*Ap[i].
// Used for the initial residual (cg.cc:79-81), the DEBUG verification (cg.cc:146-147) and the probes.
hipError_t launch_gemv_plain(const GemvPlan &plan, const double *A, long lda, int rows, const double *v_full,
                             const double *v_local, double *Ap, double *partials, Scalars *sc, hipStream_t s);

// K1, fused form = body of iteration k up to p.Ap (cg.cc:100-105) preceded by the tail of iteration k-1
// (cg.cc:117-132): rsnew = sum of the gathered r.r; convergence test; beta; p_new = r + beta p_old computed
// on the fly for every column (and stored once), Ap = A p_new, partials[wg] = the workgroup's part of p_new_local . Ap.
// e_start / e_stop (both or neither): bound to the dispatch itself (hipExtLaunchKernel), so their difference is the
// kernel's own begin -> end as rocprofv3 sees it, with no marker packets on the stream.
// plan.split > 1: Ap is the first of plan.split partial vectors, ap_stride doubles apart (piece s of the columns
// writes Ap + s * ap_stride); the consumer adds them in ascending order (launch_prefold_ap, or the fused P2P update).
// jacobi: the preconditioned form: seg is the replicated z = D^-1 r instead of r, laid out like r, with the
// r.z partials in its tail and the r.r partials behind them (at seg.base + seg.S); the head takes beta from r.z and the break
// from r.r.  The loop over A is the same code.
hipError_t launch_gemv_fused(const GemvPlan &plan, const double *A, long lda, int rows, int row0,
                             const double *p_old, double *p_new, SegView seg, double *Ap, double *partials,
                             Scalars *sc, int k, double tol, hipStream_t s, hipEvent_t e_start = nullptr,
                             hipEvent_t e_stop = nullptr, long ap_stride = 0, bool jacobi = false);
// ---- K1 for an exactly symmetric A on one GPU (plan variant 6, cgx_symv.hip) ----------------------------------------------
// A p from the upper triangle's B x B tiles: each off-diagonal tile is read once and used twice.  The plan's fields mean:
// R = tile edge B, U = tiles of the longest workgroup run, waves = 4, light = fold workgroups (= p.Ap partials in the tail),
// split = nb (blocks of B rows = slots per row of the partial buffer, nb x lda doubles, zeroed when made), grid = workgroups of
// the tile kernel, ncols as for variant 1.
constexpr int kSymvTile = 256;
constexpr int kSymvMinN = 16384;   // the default plan takes variant 6 only above this n
// run = tiles per workgroup of the static split: grid = tiles / run (runs of the grid differ by one tile at most); run = 0: the
// grid of 4 workgroups per CU (gemv_variant 60000).  The tile kernel takes its run from gridDim.x: the same kernel, the same
// bits, whatever the grid.
constexpr int kSymvRun = 1;
GemvPlan plan_symv(int n, long lda, int cus, int run = kSymvRun);
// p.Ap partials a plan's launch leaves in the tail (variant 6: one per fold workgroup; otherwise one per K1 workgroup)
inline int plan_partials(const GemvPlan &pl) { return pl.variant == 6 ? pl.light : pl.grid / (pl.split > 1 ? pl.split : 1); }
// Plain form: Ap = A v (rows < n), partials[wg] = the fold workgroup's part of v . Ap.
hipError_t launch_symv_plain(const GemvPlan &pl, const double *A, long lda, int n, const double *v, double *parts, double *Ap,
                             double *partials, hipStream_t s);
// Fused form: the contract of launch_gemv_fused on one shard (iteration head, p_new = r + beta p_old stored once, Ap, one p.Ap
// partial per fold workgroup, nothing stored once converged).  Two dispatches: e_start is bound to the tile kernel's, e_stop to
// the fold's, so the pair spans all the work that produces Ap.
hipError_t launch_symv_fused(const GemvPlan &pl, const double *A, long lda, int n, const double *p_old, double *p_new, SegView seg,
                             double *parts, double *Ap, double *partials, Scalars *sc, int k, double tol, hipStream_t s,
                             hipEvent_t e_start = nullptr, hipEvent_t e_stop = nullptr, bool jacobi = false);
// *mismatch |= 1 unless A (n x n at pitch lda) equals its transpose bit for bit (64-bit words; *mismatch zeroed by the caller).
hipError_t launch_symmetric_check(const double *A, long lda, int n, int *mismatch, hipStream_t s);

// Chunks of a rank's Ap slice (see "Chunks" in cgx_kernels.hip): kChunkRows consecutive rows, one workgroup each.
constexpr int kChunkRows = 512;
inline int chunks_per_rank(int Sr) { return (Sr + kChunkRows - 1) / kChunkRows; }
// In front of the exchange of every multi-rank transport but the fused P2P update: dst[i] = parts[i] + parts[stride + i]
// + ... (split terms, ascending; split == 1: parts == dst, nothing is stored), i < Sr, and tail[c] = the part of
// p_sub . Ap_sub (cg.cc:105) of chunk c, p_loc = p_new + row0.  K3 then folds P x chunks_per_rank(Sr) partials instead
// of every K1 workgroup's.
hipError_t launch_prefold_ap(const double *parts, int split, long stride, int rows, int Sr, const double *p_loc, double *dst,
                             double *tail, const Scalars *sc, hipStream_t s);

// K3: p.Ap = fixed-order sum over all ranks q of the tail_count doubles at tail_off of segment q's tail;
// alpha = rsold / max(p.Ap, rsold*1e-14); x_sub += alpha p_sub (own rows); r -= alpha Ap for ALL n rows (r is
// replicated, rv = [r (lda) | one r.r partial per K3 workgroup]); the next K1's head folds the partials.  cg.cc:105-116.
// How K3 and the residual set-up make z from r_new (default: they make none).  kPrecJacobi: also z = dinv * r_new into zv (the
// layout of rv) and, per workgroup, the r.z partial into zv's tail and the r.r partial behind it (zv.base + zv.S); alpha then
// uses rho = r.z (sc->rs).  kPrecBlock: z = D_b^-1 r_new from W (block, lda: see "block Jacobi" below), stored like Jacobi's.
enum PrecKind { kPrecNone = 0, kPrecJacobi = 1, kPrecBlock = 2 };
struct UpdatePrecond {
    PrecKind kind = kPrecNone;
    const double *dinv = nullptr;
    const double *W = nullptr;
    int block = 1;
    long lda = 0;
    SegView zv{};
};
hipError_t launch_update_xr(int n, int rows, int row0, const double *p_new, SegView apv, int tail_off, int tail_count,
                            double *x, SegView rv, Scalars *sc, int parity, double *partials, hipStream_t s,
                            hipEvent_t e_start = nullptr, hipEvent_t e_stop = nullptr,   // optional: bound to the dispatch
                            const UpdatePrecond &pc = UpdatePrecond{});
int update_xr_grid(int count);   // ceil(count/256), at most kMaxVectorGrid (above that the kernels stride over the rows)
constexpr int kMaxVectorGrid = 1024;

// Tail of the LAST executed iteration when the loop runs out (k = number of iterations done):
// rsnew -> rs[k&1], convergence test (cg.cc:117-121,132).  One thread.
hipError_t launch_close_iteration(Scalars *sc, SegView seg, int k, double tol, hipStream_t s, bool jacobi = false);

// K2: out[0..NV) = deterministic sum of partials (stand-alone form, setup/verification only).
hipError_t launch_reduce_partials(const double *partials, int n, double *out, hipStream_t s);
hipError_t launch_reduce_partials3(const double *partials, int n, double *out3, hipStream_t s);

// Initial residual (cg.cc:79-85): r = b - Ap for all n rows (Ap from the gathered segments); rv tail[wg] = sum r_i^2.
// Preconditioned (pc.kind): also z0 from r0 into pc.zv, the r.z partials in its tail and the r.r partials behind them.
hipError_t launch_init_residual(int n, const double *b_full, SegView apv, SegView rv, double *partials, hipStream_t s,
                                const UpdatePrecond &pc = UpdatePrecond{});

// ---- Jacobi -------------------------------------------------------------------------------------------
// dst[i] = A(row0 + i, row0 + i) for the shard's rows (dst: its Ap slice, which the segment exchange then gathers).
hipError_t launch_diag_slice(const double *A, long lda, int rows, int row0, double *dst, hipStream_t s);
// From the gathered slices: dinv[c] = 1 / a_cc for c < n, 0 up to lda; *bad = min(*bad, first row whose a_cc is not finite and
// > 0) (the caller sets *bad = INT_MAX before).
hipError_t launch_jacobi_dinv(SegView apv, int n, long lda, double *dinv, int *bad, hipStream_t s);

// ---- block Jacobi -------------------------------------------------------------------------------------
// z = D_b^-1 r, D_b = the block x block diagonal blocks of A over the global ranges [j block, min((j+1) block, n)).  The inverses:
// W[t * lda + i] = (D_b^-1)(i, s(i) + t), s(i) = i - i mod block; block x lda doubles per shard, replicated like dinv, zero
// outside the truncated last block and in the pad rows.  launch_update_xr / launch_init_residual with kind kPrecBlock run the
// block forms: z_i = one fma chain from +0.0 over t ascending, the same in every kernel.
constexpr int kBjMaxBlock = 256;   // every allowed block divides the 256 rows of an update workgroup
constexpr int kBjLdsBlock = 128;   // up to here the inversion works on a copy of the block in LDS
bool bj_block_ok(int block);       // 1, 2, 4, ..., kBjMaxBlock
// Extraction: dst[y * dst_stride + i] = A(row0 + i, s(row0 + i) + t0 + y) for y < nt, i < rows; 0 where the column is >= n.
hipError_t launch_bj_col_slice(const double *A, long lda, int n, int rows, int row0, int block, int t0, int nt, double *dst,
                               long dst_stride, hipStream_t s);
// Inversion in place, one workgroup per block, from the LOWER triangles (no pivoting; the result is mirrored: symmetric bit for
// bit).  A pivot that is not finite and > 0: *bad = min(*bad, the block's first row).
hipError_t launch_bj_invert(double *W, long lda, int n, int block, int *bad, hipStream_t s);

// ---- pivoted-Cholesky low-rank preconditioner (cgx_lowrank.hip) -------------------------------------------
// One GPU, dense storage: A ~ L L^T + delta I, z = (r - L C^-1 L^T r) / delta with C = delta I + L^T L.  L[u * lda + i] is column-
// major at the matrix pitch, rank x lda doubles, zero in the pad rows.  Rows run in tiles of 256, one workgroup each: lr_grid(n)
// = ceil(n / 256) workgroups, at most kMaxVectorGrid (n <= 262144: every dense problem that fits the device).
constexpr int kLrMaxRank = 256;        // = CGX_MAX_PRECOND_RANK
constexpr int kLrLd = 256;             // pitch of C (rank x rank) and of the partials of t = L^T r (one row per workgroup)
constexpr int kLrArmed = 0x7f7f7f7f;   // LrHead's ints as the host arms them (hipMemset 0x7f) in front of a set-up
struct LrHead {
    double delta;       // the shift in use (k_lr_delta)
    int bad_step;       // the step whose pivot was not finite and > 0 (kLrArmed: none) ...
    int bad_row;        // ... and its row; bad_step still armed: the row of a diagonal entry of A that is not finite and > 0
    int delta_bad;      // delta is not finite and > 0
    int pad;
};
struct LrWork {
    double *d;          // lda: the remaining diagonal, -inf once a row is chosen
    double *cand_v;     // 2 x kMaxVectorGrid: per-workgroup (value, index) candidates of the pivot search, ping-pong over the steps
    int *cand_i;
    int *piv;           // kLrMaxRank: the pivot rows in the order chosen
    double *C;          // kLrLd x kLrLd: C, then C^-1 in place (symmetric bit for bit)
    double *tpart;      // lr_grid(n) x kLrLd: the loop's partials of t
    LrHead *head;
};
int lr_grid(int n);
// Set-up, all on the device and in stream order: init (diagonal, first candidates), one step per column t = 0 ... rank-1 (pivot
// = the largest remaining diagonal, ties to the smallest index; column t of L; the next candidates), finish (delta = shift if
// > 0, else the mean remaining diagonal; C = delta I + L^T L).  The caller then inverts C with launch_bj_invert and reads the
// head once.  A failed step stops the later ones (they return at once).
hipError_t launch_lr_init(const double *A, long lda, int n, const LrWork &w, hipStream_t s);
hipError_t launch_lr_step(const double *A, long lda, int n, int t, double *L, const LrWork &w, hipStream_t s);
hipError_t launch_lr_finish(const double *L, long lda, int n, int rank, double shift, const LrWork &w, hipStream_t s);
// The loop: the PCG update kernel (launch_update_xr's Jacobi form on one GPU: fold of tail_count p.Ap partials in K3's order,
// x, r, the r.r partial at zv.base + zv.S) which also leaves the partials of t; then the apply kernel: z into zv, the r.z
// partials into its tail.  _init: the partials of t and of r.r from r as it is (set-up from x0).  sc == nullptr: no done flag.
hipError_t launch_lr_update(int n, const double *p_new, SegView apv, int tail_count, double *x, double *r, Scalars *sc, int parity,
                            const double *L, long lda, int rank, SegView zv, const LrWork &w, hipStream_t s,
                            hipEvent_t e_start = nullptr, hipEvent_t e_stop = nullptr);
hipError_t launch_lr_update_init(int n, double *r, const double *L, long lda, int rank, SegView zv, const LrWork &w, hipStream_t s);
hipError_t launch_lr_apply(int n, const double *r, const double *L, long lda, int rank, SegView zv, const LrWork &w,
                           const Scalars *sc, hipStream_t s);

// v_full[c] = segment value of column c (c < n), 0 for the pad: turns gathered slices into a replicated vector.
hipError_t launch_unpack_segments(SegView seg, double *v_full, long lda, hipStream_t s);

// dst[0..count) = src[0..count) by a kernel; dst or src may be pinned host memory.
hipError_t launch_copy_doubles(double *dst, const double *src, long count, hipStream_t s);

// DEBUG block (cg.cc:144-151): partials[3*wg + {0,1,2}] = sum (Ax-b)^2, b^2, x^2 over this shard's rows.
hipError_t launch_debug_norms(int count, const double *Ax, const double *b, const double *x, double *partials,
                              hipStream_t s);

// generate_lap2d_matrix (cg.cc:159-188) for rows [row0,row0+rows) straight into device memory; pad columns = 0.
hipError_t launch_generate_lap2d(double *A, long lda, int size, int row0, int rows, hipStream_t s);

// ---- dense, incompressible test data (TEST PROBE, cgx_probe_fill_matrix_hash; not a reference function) -------------
// The reference's generator leaves 5 non-zeros per row (cg.cc:178-186): at N = 32768 the matrix K1 streams is 99.985 % zeros.
// Its GEMV is a general dense dgemv (cg.cc:101-102), so parity and rate are also shown on a block in which every element is
// a different number with a full random mantissa: element (i, j) is a pure function of (seed, i, j) -- a counter-based
// hash, the splitmix64 finaliser -- so the device fills 8 GiB in place and the parity checker (which restates the
// same three lines) rebuilds any row on the host without an n x n copy.  Every step is exact in fp64, so host and device
// agree bit for bit: (h >> 11) is a 53-bit integer, * 2^-52 lands in [0, 2), - 1 in [-1, 1).
__host__ __device__ inline unsigned long long hash_mix64(unsigned long long z)
{
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// The Rademacher sign of element elem of library probe `probe` (include/cgx.h): the top bit of that hash; seed_mixed = hash_mix64(seed).
__host__ __device__ inline double rademacher_sign(unsigned long long seed_mixed, unsigned long long probe, unsigned long long elem)
{
    return (hash_mix64(seed_mixed ^ ((probe << 32) | elem)) >> 63) ? -1.0 : 1.0;
}
// symmetric: (i, j) and (j, i) give the same value.  diag != 0: A(i,i) = diag (with symmetric and diag above the spectral
// radius ~ 2 sqrt(n/3) of the off-diagonal part the block is SPD, so that CG runs on it for hundreds of iterations).
__host__ __device__ inline double hash_entry(unsigned long long seed_mixed, int symmetric, double diag, long i, long j)
{
    if (i == j && diag != 0.0) return diag;
    const unsigned long long a = (symmetric && j < i) ? (unsigned long long)j : (unsigned long long)i;
    const unsigned long long b = (symmetric && j < i) ? (unsigned long long)i : (unsigned long long)j;
    const unsigned long long h = hash_mix64(seed_mixed ^ ((a << 32) | b));
    return (double)(h >> 11) * 0x1.0p-52 - 1.0;
}
// rows [row0, row0+rows) of the n x n hash matrix into a dense block at pitch lda; pad columns = 0.
hipError_t launch_fill_hash(double *A, long lda, int n, int row0, int rows, unsigned long long seed, int symmetric, double diag,
                            hipStream_t s);

// Matrix::read (matrix.cc:12-21) on the device, for the WHOLE entry list of the file in file order (0-based I, J;
// `sym`: entry z also assigns (J,I) right after (I,J), matrix.cc:18-20).  Entries outside rows [row0,row0+rows) are
// skipped.  A later assignment to the same element overrides an earlier one exactly as the sequential loop does:
// three passes -- claim (64-bit atomic max of the assignment's sequence number into the element's own storage),
// resolve (which assignment holds the element), write (the holder stores its value) -- no sort, no host-side map.
// The block must be zero-filled before.  dv == nullptr: dense block A (rows x lda); else banded storage.
struct DiaView;
hipError_t launch_coo_assign(double *A, long lda, const DiaView *dv, double *dia_vals, int n, int row0, int rows,
                             const int *I, const int *J, const double *a, long nz, int sym, unsigned char *win /* 2*nz */,
                             hipStream_t s);

// ---- banded storage (opt-in, NOT the reference's dense contract: SURVEY.md section 8f.3) ------------------
// The row block as its non-zero diagonals: vals[t*ld + i] = A(row0+i, row0+i+off[t]) for local row i, exactly 0
// where that column lies outside [0,n).  Offsets ascending, so a row is summed in ascending column order.
constexpr int kMaxDiags = 64;
struct DiaView {
    const double *vals;
    long ld;              // >= rows
    int ndiag;
    int off[kMaxDiags];
};
GemvPlan plan_dia(int rows, int variant = 0);   // variant 3, grid = min(ceil(rows/512), 2048); plan.light = LDS-window form
                                                // (cfg variant 30001 / 30002 force the direct / the window form)

// K1 on banded storage: same contract as launch_gemv_plain / launch_gemv_fused (same iteration head, same p_new
// = r + beta p_old, same one partial per workgroup), 8*(rows*ndiag) bytes of matrix instead of 8*rows*n.
hipError_t launch_spmv_dia_plain(const GemvPlan &plan, const DiaView &dv, int rows, int row0, int n, long lda,
                                 const double *v_full, double *Ap, double *partials, Scalars *sc, hipStream_t s);
hipError_t launch_spmv_dia_fused(const GemvPlan &plan, const DiaView &dv, int rows, int row0, int n, long lda,
                                 const double *p_old, double *p_new, SegView seg, double *Ap, double *partials,
                                 Scalars *sc, int k, double tol, hipStream_t s, hipEvent_t e_start = nullptr,
                                 hipEvent_t e_stop = nullptr);
// generate_lap2d_matrix (cg.cc:159-188) straight into banded storage; dv.off must be lap2d_offsets(size).
int lap2d_offsets(int size, int *off /* >= 5 */);
hipError_t launch_dia_generate_lap2d(double *vals, const DiaView &dv, int size, int row0, int rows, hipStream_t s);
// dense row block -> which diagonals hold a non-zero: flags[(j - i_global) + (n-1)] = 1
hipError_t launch_dia_mark(const double *A, long lda, int n, int row0, int rows, unsigned char *flags, hipStream_t s);
// dense row block -> banded storage for the offsets in dv
hipError_t launch_dia_pack(const double *A, long lda, int n, int row0, int rows, double *vals, const DiaView &dv,
                           hipStream_t s);
// ---- CSR storage (opt-in, cgx_csr.hip) -----------------------------------------------------
// The row block as compressed sparse rows: row_ptr[0..rows] (local, row_ptr[0] = 0), col[] global column indices strictly
// ascending within a row, vals[] the entries as given.
struct CsrView {
    const long long *row_ptr;
    const int *col;
    const double *vals;
    long long nnz;
};
constexpr int kCsrVariantBase = 70000;   // cfg.gemv_variant 70000 + L forces L lanes per row (L = 1, 2, 4, ..., 64)
// plan variant 7: R = L lanes per row, U = entries in flight per lane, waves = 4, grid = min(ceil(rows / 64), 2048) (a function
// of rows only, so the exchange segment's geometry never depends on the matrix), rows_per_wg = 256 / L per pass.
GemvPlan plan_csr(int rows, long long nnz, int variant);
// variant <= 0 (the default) or 70000 + a power of two up to 64
bool csr_variant_ok(int variant);
// K1 on CSR storage: the contract of launch_spmv_dia_plain / launch_spmv_dia_fused, plus the Jacobi form (seg = z).
hipError_t launch_spmv_csr_plain(const GemvPlan &plan, const CsrView &cv, int rows, int row0, long lda, const double *v_full,
                                 double *Ap, double *partials, hipStream_t s);
hipError_t launch_spmv_csr_fused(const GemvPlan &plan, const CsrView &cv, int rows, int row0, long lda, const double *p_old,
                                 double *p_new, SegView seg, double *Ap, double *partials, Scalars *sc, int k, double tol,
                                 hipStream_t s, hipEvent_t e_start = nullptr, hipEvent_t e_stop = nullptr, bool jacobi = false);
// generate_lap2d_matrix (cg.cc:159-188) straight into CSR: the non-zero entries of rows [row0, row0+rows), ascending columns.
long long lap2d_csr_nnz(int size, int row0, int rows);
hipError_t launch_csr_generate_lap2d(long long *row_ptr, int *col, double *vals, int size, int row0, int rows, hipStream_t s);
// Jacobi set-up: dst[i] = the stored entry (row0 + i, row0 + i), or 0 where the row has none.
hipError_t launch_csr_diag_slice(const CsrView &cv, int rows, int row0, double *dst, hipStream_t s);
// Block-Jacobi set-up: launch_bj_col_slice on CSR storage (an entry the row does not store is 0).
hipError_t launch_csr_bj_col_slice(const CsrView &cv, int n, int rows, int row0, int block, int t0, int nt, double *dst,
                                   long dst_stride, hipStream_t s);

// ---- direct peer exchange (CGX_COMM_P2P): a lean all-gather over IPC-mapped mailboxes ---------------------
// Every rank owns one fine-grained mailbox; all ranks map all mailboxes.  Layout (identical on every rank):
//   flags : [kP2pChannels][kMaxRanks] words, one 128-B line each   (flag[c][q] = last epoch rank q delivered on channel c)
//   chunk flags : kMaxChunkFlags words of 8 B, word q*cpr + c = last epoch rank q delivered chunk c of its slice on
//                 channel 1 through the fused update kernel (k_update_xr_p2p)
//   data  : per channel c, [2 parities][nranks] slots of slot_bytes[c]
constexpr int kP2pChannels = 3;          // 1 = [Ap slice | p.Ap] segments, 2 = DEBUG scalars; 0 = with tagged words: the plain
                                         // all-gathers of segments (set-up / verification phases), else unused
constexpr int kP2pFlagStride = 128;      // bytes between flag words
constexpr int kMaxChunkFlags = 2048;     // nranks * chunks per rank <= this (262144 rows: 512 + nranks)
struct MailboxView {
    unsigned char *base[kMaxRanks];      // base[q] = rank q's mailbox as mapped in THIS process (base[rank] = own)
    long cflag_off;                      // byte offset of the chunk flag words
    long data_off[kP2pChannels];         // byte offset of channel c's data area
    long slot_bytes[kP2pChannels];       // bytes per (parity, rank) slot
    int nranks, rank;
    int tagged;                          // 1 = the fused update hands its bytes over as tagged words (no flags, no fences;
                                         // cgx_p2p.hip "Tagged words"); slots of channel 1 are then twice as large
    int acquire;                         // 1 = one system-scope acquire fence per workgroup behind the flag wait of
                                         // k_update_xr_p2p (default); 0 only for the A/B of its cost (tools/p2p_one_rank.py)
};

// All-gather `count` doubles per rank: rank's own contribution is src; afterwards dst + q*dst_stride holds
// rank q's for every q (own part copied from src only if copy_self).  If tail_n > 0, the fixed-order sum of
// src[tail_off .. tail_off+tail_n) travels as one extra double and lands at dst[q*dst_stride + sum_off].
// One workgroup per peer: push my data + release + flag into the peer's mailbox, wait (bounded) for the peer's
// flag in mine, copy its data out.
hipError_t launch_mailbox_allgather(const MailboxView &mv, int chan, unsigned long long epoch, const double *src,
                                    int count, int tail_off, int tail_n, double *dst, long dst_stride, int sum_off,
                                    int copy_self, long long timeout_ticks, int *err, hipStream_t s);

// K3 with the iteration's exchange inside (CGX_COMM_P2P): the (peer, chunk) pairs are dealt over the workgroups, each
// pushes [one chunk of the Ap slice | its p.Ap partial] into one peer's mailbox and raises that peer's chunk flag; every
// workgroup waits (bounded) for all nranks x cpr flags and reads the Ap element of its row and the partials straight from
// the mailbox.  The iteration is then K1 + this kernel.  ap_src: this rank's Ap slice as `split` column pieces of K1,
// `stride` apart (split == 1: the whole slice), added up in ascending order on the fly.  cpr = chunks_per_rank(apv.Sr).
hipError_t launch_update_xr_p2p(int n, int rows, int row0, const double *p_new, SegView apv, int cpr,
                                const MailboxView &mv, int chan, unsigned long long epoch, double *x, SegView rv, Scalars *sc,
                                int parity, long long timeout_ticks, int *err, hipStream_t s,
                                const double *ap_src, int split, long stride, hipEvent_t e_start = nullptr,
                                hipEvent_t e_stop = nullptr, const double *dinv = nullptr, SegView zv = SegView{});
// The exchange of launch_update_xr_p2p alone (the same kernel template, SELFTEST = true), on caller data: vals[i] = the Ap
// element read for global row i (n doubles), sums[wg] = the folded chunk partials as workgroup wg saw them
// (update_xr_grid(n) doubles).
hipError_t launch_chunk_exchange_selftest(int n, int rows, int row0, const double *p_like, SegView apv, int cpr,
                                          const MailboxView &mv, int chan, unsigned long long epoch, long long timeout_ticks,
                                          int *err, const double *ap_src, int split, long stride, double *vals, double *sums,
                                          hipStream_t s);
// Workgroups of k_update_xr_p2p the device keeps resident at once (occupancy x CUs): its grid must not exceed this, since
// its workgroups wait for each other inside the kernel.
hipError_t update_xr_p2p_resident_limit(int device, bool tagged, int *workgroups);

// ---- the LDS-resident solver for small dense problems (cgx_resident.hip) ----------------------------------------------
// n <= 2048 on one GPU: the row groups of A live in the CUs' LDS for the whole launch, x / r / p are replicated in every
// workgroup's registers, and the loop cg.cc:95-137 runs inside ONE persistent kernel whose workgroups exchange Ap as tagged
// words (no grid barrier).  All workgroups wait for each other: the grid never exceeds the number of CUs.
struct ResidentPlan {
    int R;             // rows per workgroup: the power of two with R x min(CUs, 256) >= n (<= 8)
    int S;             // column steps of 512
    int rows_per_wg;   // = R
    int grid;          // workgroups = ceil(n / R) <= CUs
    int xslots;        // tagged doubles per parity of the exchange buffer (512 * S)
    size_t lds_bytes;  // dynamic LDS of one workgroup
    int hybrid;        // 1 = 2048 < n <= 4096: R = 16 rows per workgroup, of which RL in LDS, RG in registers and
    int RL, RG;        //     R - RL - RG streamed from memory every iteration; 0: all R rows in LDS (RL = R, RG = 0)
    int stream;        // 1 = cgx_stream.hip (4096 < n <= 16384): workgroups of 512 threads, S = column steps of 1024, every row
    int RB;            //     streamed through a ring of RB rows; of the R rows per workgroup the first RL stay in LDS and the next RG in
                       //     registers, the other R - RL - RG (a multiple of RB) are streamed every iteration
    int l2_rows;       //     ... the first l2_rows of them with the default cache policy (they stay in the XCD's L2), the others nt
};
// One block of solver state (x | r + the update kernel's r.r partials | p | Scalars), offsets in doubles from its base.  On one
// GPU the shard keeps TWO such blocks (cgx_context.cpp): the persistent kernels read one and write the other.
constexpr long kStateTail = 1024;   // = kMaxVectorGrid: room for one r.r partial per workgroup of the update kernel behind r
__host__ __device__ inline long state_off_r(long lda) { return lda; }
__host__ __device__ inline long state_off_p(long lda) { return 2 * lda + kStateTail; }
__host__ __device__ inline long state_off_sc(long lda) { return 3 * lda + kStateTail; }
__host__ __device__ inline long state_doubles(long lda) { return 3 * lda + kStateTail + 16; }   // Scalars: 96 bytes
// What a persistent launch reports to the host, written by the kernel straight into pinned host memory (so that a solve needs no
// copy command for it): workgroup 0 writes the head and, LAST, the launch's stamp -- it does so on every path out of the kernel,
// also when a wait expired or the error word was already up when it started, and since a kernel is over only when all of its
// workgroups are, the host finds the stamp of THIS launch behind the stream's synchronisation whatever happened.  Every
// workgroup writes its own line of `waits` (all of them fresh after any launch that has ended).
struct ResidentTail {
    int done, k_final;     // the break of cg.cc:120-121 was taken, in iteration k_final
    int err;               // a bounded wait expired (or the error word was up at the start)
    unsigned stamp;        // ResidentArgs::stamp of the launch that wrote this
    // workgroup 0: iterations run | polls of the watched word that had to be repeated | gather rounds that had to be repeated
    long long iterations, watch_repeats, gather_repeats;
    // per workgroup, 100-MHz ticks: from its publish of the launch's FIRST iteration until it had gathered all of Ap (a workgroup
    // that was placed late shows here) | the longest such span of a LATER iteration in which a poll had to be repeated (0: none)
    unsigned waits[256][2];
};
struct ResidentArgs {
    const double *A;   // n x lda, row-major, pad columns zero
    long lda;
    int n, rows_per_wg, xslots;
    const double *in;  // the state the launch STARTS from, one block laid out by state_off_*: x | r | p | Scalars (p is read only
                       // when k0 > 0; rs[] in the per-launch path's convention) -- never written: a launch whose waits expire
                       // leaves all of it intact and the host redoes it on the per-launch path
    double *out;       // the state the launch ENDS with, a second block of the same layout (the host makes it the current one
                       // after a launch that came back without the error word raised): x, r, p, rs[], done, k_final
    unsigned long long *xbuf;   // device memory, 2 parities x xslots x 2 words, zero-filled when the problem is set
    unsigned long long epoch0;  // the launch uses epochs epoch0 + 1 ... epoch0 + iters
    int k0, iters;     // iterations k0 ... k0 + iters - 1 (stops at the break of cg.cc:120-121)
    double tol;
    long long timeout_ticks;    // bound of every wait, 100 MHz wall-clock ticks
    int *err;          // device word raised when a wait expired
    int l2_rows;       // streaming kernel: the first l2_rows streamed rows of every workgroup are read with the default cache policy (the others nt)
    int stagger;       // streaming kernel: every workgroup begins its sweep at a batch of its own (0 = all at their first rows)
    int mute_wg;       // test only (cgx_probe_resident_test): this workgroup leaves out the publish of the launch's first iteration; -1 = none
    ResidentTail *tail;   // PINNED HOST memory: what the launch reports back (written by the kernel itself: no copy command)
    unsigned stamp;    // the launch's number (never 0): workgroup 0's last word into the tail
    long long *prof;   // diagnostics (CGX_RESIDENT_PROFILE=1), else nullptr: workgroup 0 adds up shader-clock cycles per phase
                       // [0] GEMV + row sums + publish, [1] wait for the watched word, [2] gather, [3] p.Ap, [4] update + r.r,
                       // [5] watch rounds, [6] gather rounds, [7] iterations
};
// false: this problem does not fit (n > 16384, too few CUs, LDS per workgroup too small).  n <= 4096: the matrix stays on
// the chip (cgx_resident.hip); above: every row is streamed (cgx_stream.hip, plan_stream).
bool plan_resident(int n, int cus, size_t lds_per_wg, ResidentPlan *out);
// The streaming persistent kernel alone (1024 <= n <= 16384; tests force it below 4096 too): plan, and prepare (a == nullptr:
// raise the dynamic-LDS limit, *per_cu = workgroups the runtime keeps resident per CU) / launch.
bool plan_stream(int n, int cus, size_t lds_per_wg, ResidentPlan *out);
hipError_t stream_dispatch(const ResidentPlan &pl, const ResidentArgs *a, hipStream_t s, int *per_cu);
// Once per plan, before the first launch: raises the kernel's dynamic-LDS limit; *workgroups_per_cu = what the runtime
// keeps resident per CU (the caller checks grid <= that x CUs: the workgroups wait for each other).
hipError_t prepare_cg_resident(const ResidentPlan &pl, int *workgroups_per_cu);
hipError_t launch_cg_resident(const ResidentPlan &pl, const ResidentArgs &a, hipStream_t s);

// ---- a persistent solve from a ZERO initial guess in four launches (n <= 16384, one GPU; cgx_solve.cpp) --------------------------
// Everything cgx_solve_begin does for x0 = 0 in ONE kernel: x = 0, r = b (b - A 0, cg.cc:79-82: A 0 is exactly 0), one r.r partial
// per 256 rows behind r (what the per-launch K1 of iteration 0 folds, should the persistent launch have to be redone), both p
// buffers, the exchanged segments and the scalar block zeroed, the error word down.
hipError_t launch_solve_begin_zero(int n, long lda, const double *b_full, double *x, SegView rv, double *p0, double *p1, double *apg,
                                   long apg_count, Scalars *sc, int *err, hipStream_t s);
// Everything cgx_solve_end does behind the verification GEMV in ONE kernel (one workgroup of 1024 threads, fixed order):
// out[0 .. n) = x, out[n + 0 .. 2] = sum (Ax - b)^2, sum b^2, sum x^2 (cg.cc:144-151), out[n + 3 .. 4] = sc->rs[0 .. 1]; out is
// pinned host memory.
hipError_t launch_solve_end(int n, const double *Ax, const double *b, const double *x, const Scalars *sc, double *out, hipStream_t s);

// Loopback "collective": copy local[kSlots] of every shard into gathered[] of every shard (<= 16 shards).
hipError_t launch_loopback_gather(double *const *gathered_ptrs, const Scalars *const *scalar_ptrs, int nshards,
                                  hipStream_t s);

// ---- several right-hand sides against one dense matrix, one GPU (cgx_multi.hip) ----------------------------------------------
// Blocks of vectors are column-major at pitch lda (column j at base + j * lda, zero padded up to lda).  nrhs columns run in the
// kernels of width multi_width(nrhs) (1, 2, 4, 8 or 16); columns nrhs .. width-1 are masked by nrhs.
constexpr int kMaxRhs = 16;   // = CGX_MAX_RHS
// One double per column, by value into a kernel: the shifts of cgx_solve_shifted / cgx_solve_minres (the rest stays 0).
struct ColumnSigmas {
    double v[kMaxRhs];
};
inline ColumnSigmas column_sigmas(const double *sigma, int count)
{
    ColumnSigmas sg{};
    for (int j = 0; j < count; ++j) sg.v[j] = sigma[j];
    return sg;
}
struct MultiScalars {
    double rs[kMaxRhs][2];     // per column: rs[j][k & 1] is rsold of iteration k (as Scalars::rs)
    int    done[kMaxRhs];      // the column took the break (cg.cc:120-121); nothing writes its x, r, p or scalars afterwards
    int    k_final[kMaxRhs];   // k of the column's converging iteration
    int    all_done;           // every column has broken: the host polls this word; later kernels exit at once
    int    k_all;
    int    pad[2];
    double norms[kMaxRhs][3];  // ||Ax - b||^2, ||b||^2, ||x||^2 per column (cg.cc:146-151; launch_column_norms)
};
struct MultiArgs {
    const double *A;
    long lda;
    int n, nrhs;
    const double *v;           // plain: the vectors; fused: p_old
    double *p_new;             // fused: p = r + beta p_old, stored once
    const double *r;           // fused: the residuals
    const double *rrp;         // fused: K3m's r.r partials, multi_update_grid(n) per column
    double *Y;                 // A v (live columns only)
    double *partials;          // multi_gemv_grid(n, width) per column: v_j . Y_j of each workgroup
    MultiScalars *ms;
    int k;
    double tol;
};
int multi_width(int nrhs);
// launch(std::integral_constant<int, W>{}) for W = multi_width(nrhs): THE dispatch over the five kernel widths
template <class Launch>
auto for_multi_width(int nrhs, Launch &&launch)
{
    switch (multi_width(nrhs)) {
    case 1: return launch(std::integral_constant<int, 1>{});
    case 2: return launch(std::integral_constant<int, 2>{});
    case 4: return launch(std::integral_constant<int, 4>{});
    case 8: return launch(std::integral_constant<int, 8>{});
    default: return launch(std::integral_constant<int, 16>{});
    }
}
int multi_rows_per_wg(int width);
int multi_gemv_grid(int n, int width);   // K1m workgroups = p.Ap partials per column
int multi_update_grid(int n);            // K3m workgroups per column = r.r partials per column
// K1m: plain (Y = A V) or fused (head of iteration k, P = R + beta P_old, Y = A P); e0 / e1 optional, bound to the dispatch.
hipError_t launch_multi_gemv(const MultiArgs &g, bool fused, hipStream_t s, hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr);
// K3m: for every live column x += alpha p, r -= alpha Y, r.r partials (grid multi_update_grid(n) x nrhs).
hipError_t launch_multi_update(int n, long lda, int nrhs, const double *p, const double *Y, const double *partials, int g1, double *x,
                               double *r, double *rrp, MultiScalars *ms, int parity, hipStream_t s);
// r = B - Y and r.r partials (set-up); the head of iteration k alone (the loop ran out).
hipError_t launch_multi_init(int n, long lda, int nrhs, const double *b, const double *Y, double *r, double *rrp, hipStream_t s);
hipError_t launch_multi_close(MultiScalars *ms, const double *rrp, int n, int nrhs, int k, double tol, hipStream_t s);
// THE end-of-solve norms of every k-column solve (cg.cc:146-151), behind the plain K1m pass (or the SpMVs) that left Y_j = A x_j:
// norms[3 j ...] = ||Y_j + sigma_j x_j - b_j||^2, ||b_j||^2, ||x_j||^2 for j < ncol, one workgroup per column, fixed order.  b_j is
// b + j * ldb: ldb = lda for a block of right-hand sides, 0 for one source term shared by all shifts.  sigma: ncol host doubles,
// or nullptr: the kernel without the sigma term (not the same as sigma = 0 where x is not finite).
hipError_t launch_column_norms(int n, long lda, int ncol, const double *Y, const double *X, const double *b, long ldb,
                               const double *sigma, double *norms, hipStream_t s);

// ---- several right-hand sides with a preconditioner (cgx_solve_multi_pc, cgx_multi_pc.hip) ----------------
// Every column runs the recurrence of section 11 on the blocks above plus Z = M^-1 R.  MultiScalars keeps its layout: rs[j][] holds
// rho_j = r_j.z_j (as Scalars::rs does under Jacobi), and r_j.r_j -- the break and the report -- lives in a block of its own.
struct MultiPcScalars {
    double rr[kMaxRhs][2];     // per column: r.r in rs's ping-pong (as Scalars::rr)
};
// The preconditioner M as the multi-column kernels take it (here and in cgx_lanczos_pc.hip); the host fills it with pc_factor
// (cgx_precond.cpp).
struct PcFactor {
    const double *dinv;        // point Jacobi: the inverse diagonal (lda doubles); nullptr = pivoted Cholesky:
    const double *L;           //   rank x lda, column-major at the matrix pitch
    int rank;
    const double *Cinv;        //   (delta I + L^T L)^-1 at pitch kLrLd
    const LrHead *head;        //   delta
    double *tpart;             //   kMaxRhs x lr_grid(n) x kLrLd: per column and 256-row tile the partials of t_j = L^T r_j
};
// Whether the K3m of this M can run on n rows: Jacobi always; the factor with a rank of 1 .. min(n, kLrMaxRank) and one workgroup
// per 256-row tile, lr_grid(n) = multi_update_grid(n) <= kMaxVectorGrid of them.
bool pc_factor_ok(int n, const PcFactor &f);
struct MultiPcArgs {
    double *Z;                 // kMaxRhs x lda: z_j = M^-1 r_j (live columns only)
    double *rzp;               // r.z partials, multi_update_grid(n) per column, beside MultiArgs::rrp
    MultiPcScalars *mp;
    PcFactor M;
};
// K1m fused with the preconditioned head: g.r is Z, g.rrp the r.r partials; beta_j from r.z, the break from r.r.
hipError_t launch_multi_gemv_pc(const MultiArgs &g, const MultiPcArgs &pc, hipStream_t s, hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr);
// K3m: launch_multi_update's work plus z and the r.z partials.  Jacobi: one launch (grid tiles x nrhs).  Pivoted Cholesky: two
// launches of one workgroup per 256-row tile that serve all live columns, so the tile of L is read once per launch: the update
// (x, r, r.r partials, partials of t_j) and the apply (t_j folded, u_j = C^-1 t_j, z_j, r.z partials).  init: r is taken as it is
// (the set-up behind launch_multi_init, and the probe); p, Y, partials, x are not read then and every column < nrhs counts as live.
hipError_t launch_multi_update_pc(int n, long lda, int nrhs, const double *p, const double *Y, const double *partials, int g1, double *x,
                                  double *r, double *rrp, MultiScalars *ms, int parity, const MultiPcArgs &pc, bool init, hipStream_t s);
hipError_t launch_multi_close_pc(MultiScalars *ms, const MultiPcArgs &pc, const double *rrp, int n, int nrhs, int k, double tol,
                                 hipStream_t s);

// ---- multi-shift CG: (A + sigma_j I) x_j = b for up to kMaxShifts shifts from one Krylov sequence (cgx_shift.hip) -------------
// The seed is the single path's loop on A (K1 + K3, untouched); one kernel behind each K3 advances every shift.  X and P (the
// x and p of the shifts) are column-major at pitch lda like the multi block: shift j at base + j * lda, zero padded up to lda.
constexpr int kMaxShifts = 16;                 // = CGX_MAX_SHIFTS
constexpr int kShiftLive = 0x7fffffff;         // frozen_at / all_at of a shift / a solve that is still running
struct ShiftScalars {
    double sigma[kMaxShifts];
    double zeta[3][kMaxShifts];    // zeta_m of shift j at zeta[(m + 1) % 3][j]: the launch of iteration k reads m = k, k - 1 and
                                   // writes m = k + 1, so no workgroup reads a slot another one of the same launch writes
    double alpha[3], beta[3];      // the seed's alpha_m, beta_m at [(m + 1) % 3] (alpha_-1 = 1, beta_-1 = 0)
    double res_last[kMaxShifts];   // |zeta_(k+1)| sqrt(r_(k+1).r_(k+1)) of the shift's last iteration k
    double res_prev[kMaxShifts];   // |zeta_k| sqrt(r_k.r_k)
    double norms[kMaxShifts][3];   // ||(A + sigma I) x - b||^2, ||b||^2, ||x||^2 (launch_column_norms)
    int    frozen_at[kMaxShifts];  // the iteration that froze the shift (kShiftLive: running).  An iteration number, not a flag:
                                   // workgroup 0 of launch k writes k while the others still read, and both values mean "runs in k"
    int    all_at;                 // the iteration that ended the loop (every shift frozen, or the seed broke); launches of later
                                   // iterations exit at once
    int    pad[3];
};
struct ShiftArgs {
    int n, nshift;
    long lda;
    const double *r;               // the seed's r behind K3 of iteration k: r_(k+1)
    const double *rrp;             // K3's r.r partials (the tail of the replicated r), folded as the next K1's head folds them
    int nrr;
    const double *pap;             // K1's p.Ap partials as K3 was handed them (tail offset and count), folded in K3's order
    int npap;
    int pap_strided;               // 1 = K3 ran in its strided form (more than 256 * kMaxVectorGrid rows): that form's fold order
    Scalars *sc;                   // the seed's scalar block: rs[k & 1] = rsold of iteration k; done / k_final are raised when the
                                   // loop ends, so that the seed's later kernels drain and the host's poll sees it
    ShiftScalars *ss;
    double *X, *P;
    int k;
    double tol;
};
// x_j = 0, p_j = b (zero padded up to lda) for j < nshift, and the scalar block set for iteration 0 (sigma: host array).
hipError_t launch_shift_begin(int n, long lda, int nshift, const double *sigma, const double *b, double *X, double *P, ShiftScalars *ss,
                              hipStream_t s);
// Behind K3 of iteration k: alpha_k and beta_k refolded, zeta advanced, x_j and p_j updated, freeze and loop end decided.
hipError_t launch_shift_update(const ShiftArgs &a, hipStream_t s);
// The loop ran out after k iterations: residual_prev of the shifts still running (k == 0: sqrt(r0.r0) from the partials).
hipError_t launch_shift_close(ShiftScalars *ss, const double *rrp, int nrr, int nshift, int k, hipStream_t s);

// ---- MINRES: (A + sigma_j I) x_j = b for up to kMaxMinresShifts shifts of either sign, A symmetric (cgx_minres.hip) -----------
// One Lanczos recurrence from r0 = b serves every shift.  Launch t is the plain K1 of the shard's plan on
// the not yet normalised w_t, then launch_minres_step, which finishes Lanczos step t and closes column t - 1 of every shift.
// X and D[2] (the x of the shifts and their last two search directions) are column-major at pitch lda like the shift block.
constexpr int kMaxMinresShifts = 16;           // = CGX_MAX_MINRES_SHIFTS
constexpr int kMinresLive = 0x7fffffff;        // frozen_at / end_at of a shift / a loop that is still running
static_assert(kMaxShifts == kMaxRhs && kMaxMinresShifts == kMaxRhs,
              "ColumnSigmas carries the shifts, and their verification runs the multi-vector K1 at full width");
struct MinresScalars {
    int    done;                   // the two words the host polls: raised with end_at
    int    end_at;                 // the launch that ended the loop (every shift frozen, or a breakdown); later launches exit at once
    int    pad[2];
    double alpha[2];               // alpha_t at [t & 1]: launch t reads alpha_(t-1) and writes alpha_t, never the slot another
    double amax[2];                // workgroup of the same launch reads; max over s <= t of |alpha_s| likewise
    double sigma[kMaxMinresShifts];
    // the rotation state of shift j in front of column k at [(k + 1) & 1][j]: launch t = k + 1 reads it and writes column k + 1's
    double cs[2][kMaxMinresShifts], sn[2][kMaxMinresShifts], dbar[2][kMaxMinresShifts], eps[2][kMaxMinresShifts];
    double phibar[2][kMaxMinresShifts];
    double res_last[kMaxMinresShifts];   // |phibar_(k+1)| behind the shift's last column k
    double res_prev[kMaxMinresShifts];   // |phibar_k|
    int    frozen_at[kMaxMinresShifts];  // the column that froze the shift (kMinresLive: running); a number, not a flag, as
                                         // ShiftScalars::frozen_at
    int    conv[kMaxMinresShifts];       // 1 = frozen below tol, or by a breakdown that left the shift regular
};
struct MinresArgs {
    int n, nshift;
    long lda;
    double *w, *vprev;             // launch t: w_t (becomes v_t) and v_(t-1) (becomes w_(t+1)); the host swaps them between launches
    const double *Y;               // K1's product A w_t
    const double *k1p;             // ... and its w_t . A w_t partials
    int nk1p;
    const double *ww_in;           // the ||w_t||^2 partials of launch t - 1 (t = 0: of the init kernel), update_xr_grid(n) of them
    double *ww_out;
    double *X, *D[2];              // d_m of shift j at D[m & 1] + j * lda
    MinresScalars *ms;
    int t;                         // the close kernel: the launches that were enqueued
    double tol;
};
// w_0 = b and v_-1 = 0 (zero padded up to lda), x_j = d_j = 0 for j < nshift, the ||b||^2 partials and the scalar block (sigma:
// host array).
hipError_t launch_minres_init(const MinresArgs &a, const double *sigma, const double *b, hipStream_t s);
// Behind K1 of launch t: beta_t, alpha_t, the breakdown test, column t - 1 of every running shift (x update, freeze, loop end),
// v_t, w_(t+1) and its ||.||^2 partials.
hipError_t launch_minres_step(const MinresArgs &a, hipStream_t s);
// Behind the last launch (a.t launches were enqueued): the last column with beta from the last partials, unless the loop has ended.
hipError_t launch_minres_close(const MinresArgs &a, hipStream_t s);

// ---- multi-vector Lanczos for Gauss quadrature (cgx_lanczos, cgx_trace_slq; cgx_lanczos.hip) -----------
// Up to kMaxRhs three-term recurrences side by side, blocks laid out as the multi kernels' (column j at base + j * lda, zero padded
// up to lda).  A step is the plain K1m (launch_multi_gemv, fused = false) on the not yet normalised w, then launch_lanczos_step.
constexpr int kMaxLanczosSteps = 1024;         // = CGX_MAX_LANCZOS_STEPS
constexpr int kLanczosLive = 0x7fffffff;       // LanczosScalars::m of a column that is still running
struct LanczosScalars {
    double amax[kMaxRhs][2];   // max |alpha_s| over s < t at [t & 1]: step t reads that slot and writes the other
    double z2[kMaxRhs];        // ||V0_j||^2
    int    m[kMaxRhs];         // steps the column made before it was frozen (kLanczosLive: running).  A step number, not a flag:
                               // workgroup 0 of step t writes t while the others still read, and both values mean "decides in t"
    int    bad[kMaxRhs];       // the start vector has norm 0 or is not finite (m = -1: no step runs)
};
struct LanczosArgs {
    int n, nvec;
    long lda;
    double *w;                 // in: the unnormalised w_t;   out: v_t = w_t / beta_(t-1)
    double *vprev;             // in: v_(t-1);                out: the unnormalised w_(t+1)
    const double *Y;           // K1m's A w_t
    const double *k1p;         // K1m's w_t . A w_t partials, g1 per column
    int g1;
    const double *ww_in;       // ||w_t||^2 partials, multi_update_grid(n) per column
    double *ww_out;            // ||w_(t+1)||^2 partials
    LanczosScalars *ls;
    double *alpha, *beta;      // the histories: kMaxRhs rows of kMaxLanczosSteps
    int t;
};
// Per column (one workgroup each): ||V0_j||^2 in a fixed order as the column's one ||w||^2 partial, v_(-1) = 0, the scalars reset;
// a zero or non-finite column is marked bad and never runs.
hipError_t launch_lanczos_init(int n, long lda, int nvec, const double *w, double *vprev, double *ww, LanczosScalars *ls, hipStream_t s);
// Step t behind K1m: beta_(t-1) and the breakdown test, alpha_t, v_t over w, w_(t+1) over v_(t-1), the next ||w||^2 partials.
hipError_t launch_lanczos_step(const LanczosArgs &a, hipStream_t s);
// Behind the last step: beta_(steps-1) and m = steps for the columns still running.
hipError_t launch_lanczos_close(int n, int nvec, int steps, const double *ww, LanczosScalars *ls, double *beta, hipStream_t s);

// ---- the same with a preconditioner (cgx_lanczos_pc, cgx_trace_slq_pc; cgx_lanczos_pc.hip) ----------------
// Per column w (the side of M), u = M^-1 w and v_prev; K1m runs on the not yet normalised u.  LanczosScalars keeps its meaning with
// z2 = eta0^2 = w_0 . M^-1 w_0.  M.dinv != nullptr: point Jacobi, one launch per step (grid tiles x nvec); else the pivoted-Cholesky
// factor, two launches of one workgroup per 256-row tile that serve every live column (the step, then the apply).
struct LanczosPcArgs {
    int n, nvec;
    long lda;
    double *w;                 // in: the unnormalised w_t;   out: v_t = w_t / beta_(t-1)
    double *vprev;             // in: v_(t-1);                out: the unnormalised w_(t+1)
    double *u;                 // in (K1m's operand): u_t;    out: u_(t+1) = M^-1 w_(t+1)
    const double *Y;           // K1m's A u_t
    const double *k1p;         // K1m's u_t . A u_t partials, g1 per column
    int g1;
    const double *wu_in;       // w_t . u_t partials, multi_update_grid(n) per column
    double *wu_out;            // w_(t+1) . u_(t+1) partials
    LanczosScalars *ls;
    double *alpha, *beta;      // the histories: kMaxRhs rows of kMaxLanczosSteps
    int t;
    PcFactor M;                // tpart: the partials of t_j = L^T w_j
};
// The set-up from w = V0 as it is: u_0 = M^-1 w_0, v_-1 = 0, the w_0 . u_0 partials into wu_out, and per column eta0^2 folded in the
// steps' order and the scalars reset; a column whose eta0^2 is 0, negative or not finite is marked bad and never runs.
hipError_t launch_lanczos_pc_init(const LanczosPcArgs &a, hipStream_t s);
// Step t behind K1m: beta_(t-1) and the breakdown test, alpha_t, v_t over w, w_(t+1) over v_(t-1), u_(t+1), the next partials.
hipError_t launch_lanczos_pc_step(const LanczosPcArgs &a, hipStream_t s);
// Behind the last step: beta_(steps-1) and m = steps for the columns still running.
hipError_t launch_lanczos_pc_close(int n, int nvec, int steps, const double *wu, LanczosScalars *ls, double *beta, hipStream_t s);
// nprobe probes (probe0, probe0 + 1, ... of the seed) into Z (column j at + j * lda): kind 0 = cgx_trace_slq's Rademacher signs
// (covariance I); kLpcJacobi: sign_i sqrt(A_ii); kLpcLowrank: L g + sqrt(delta) sign with g_c the sign of element n + c
// (covariance M = the preconditioner, exactly).
constexpr int kLpcJacobi = 1, kLpcLowrank = 2;
hipError_t launch_lanczos_pc_probes(int n, long lda, int nprobe, int kind, unsigned long long seed_mixed, int probe0, const double *A,
                                    const double *L, int rank, const LrHead *head, double *Z, hipStream_t s);

// ---- a matrix function applied to vectors (cgx_apply_function; cgx_funm.hip) -------------------------------
// X_j[i] = sum over t < m[j] of C[j * steps + t] * Q[(t * nvec + j) * lda + i], one fma chain per element in ascending t from +0.0.
struct FunmArgs {
    int n, nvec, steps;
    long lda;
    const double *Q;           // the kept Lanczos basis: steps slots of nvec x lda doubles; slots at t >= m[j] are never read
    const double *C;           // nvec rows of `steps` coefficients
    const int *m;              // nvec step counts, 0 .. steps
    double *X;                 // nvec x ldx
    long ldx;
};
hipError_t launch_funm_combine(const FunmArgs &a, hipStream_t s);

// ---- extreme eigenpairs by Lanczos with full reorthogonalisation (cgx_eigenpairs; cgx_eigs.hip) ------------
// One start vector; the basis keeps one vector per slot, element i of q_s at Q[s * lda + i], steps + 1 slots.  A step is the plain
// K1m at width 1 on slot t, then project(first) / subtract / project / subtract(second) / normalise.
constexpr int kMaxEigenpairs = 16;             // = CGX_MAX_EIGENPAIRS
constexpr int kEigsLive = 0x7fffffff;          // EigsScalars::m of a run that is still going
constexpr int kEigsTile = 256;                 // rows per workgroup of the step kernels, = rows per projection partial
constexpr int kEigsChunk = 32;                 // slots per projection workgroup (4 waves x 8)
constexpr int kEigsSlotPitch = 1040;           // doubles per tile in the projection partials: kMaxLanczosSteps slots, 128-B lines
struct EigsScalars {
    double amax[2];            // max |alpha_s| over s < t at [t & 1]: step t reads that slot and writes the other
    double z2;                 // ||v0||^2
    int    m;                  // steps made before the run was frozen (kEigsLive: running; -1: bad start vector).  A step number,
                               // not a flag, as LanczosScalars::m
    int    bad;                // the start vector has norm 0 or is not finite
};
struct EigsArgs {
    int n;
    long lda;
    int t;                     // the step; project / subtract run on slots 0 .. t
    double *Q;                 // the basis
    const double *Y;           // K1m's A q_t
    double *W;                 // lda: the vector under orthogonalisation
    const double *k1p;         // K1m's q_t . A q_t partials
    int g1;
    double *hp;                // eigs_tiles(n) x kEigsSlotPitch: the projection partials, [tile][slot]
    double *h;                 // kEigsSlotPitch: the folded h of the latest subtraction (the probe reads it)
    double *wwp;               // eigs_tiles(n): the ||w||^2 partials of the second subtraction
    double *alpha, *beta;      // the histories, kMaxLanczosSteps each
    EigsScalars *sc;
};
int eigs_tiles(int n);
// q_0 = v0 / ||v0|| in place (n doubles at q0), the scalars reset; a zero or non-finite v0 is marked bad and no step runs.
hipError_t launch_eigs_init(int n, double *q0, EigsScalars *sc, hipStream_t s);
// first: alpha_t, w = y - alpha_t q_t - beta_(t-1) q_(t-1) into W, and the partials of Q_t^T w; else the partials from W as it is.
hipError_t launch_eigs_project(const EigsArgs &a, bool first, hipStream_t s);
// h folded in ascending tile order, W -= Q_t h; second: also the ||w||^2 partials.
hipError_t launch_eigs_subtract(const EigsArgs &a, bool second, hipStream_t s);
// beta_t, the breakdown test, q_(t+1) = W / beta_t into slot t + 1.
hipError_t launch_eigs_normalise(const EigsArgs &a, hipStream_t s);
// X_j[i] = sum over t < m of C[t * width + j] q_t[i], j < nev, width = multi_width(nev): the basis is read once for all vectors.
hipError_t launch_eigs_combine(int n, long lda, int m, int nev, const double *Q, const double *C, double *X, long ldx, hipStream_t s);
// out[j] = || Y_j - theta_j X_j ||^2, one workgroup per vector, fixed order.
hipError_t launch_eigs_residual(int n, long lda, int nev, const double *Y, const double *X, const double *theta, double *out,
                                hipStream_t s);

}  // namespace cgx
