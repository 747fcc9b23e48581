// cgx_device.h -- device-side helpers shared by the kernel translation units (cgx_kernels.hip, cgx_p2p.hip, cgx_symv.hip,
// cgx_resident.hip): the fixed-order reductions, the safeguard of alpha, the tagged-word store, the iteration head of the
// per-launch GEMV kernels, and the chunk arithmetic in front of every multi-rank exchange.  Device code only.
#pragma once

#include <hip/hip_runtime.h>

#include <type_traits>

#include "cgx_kernels.h"

namespace cgx {

typedef double d2 __attribute__((ext_vector_type(2)));

static constexpr double kNearZero = 1.0e-14;   // NEARZERO, code/MPI/cg.cc:8

// alpha = rsold / std::max(conj, rsold * NEARZERO), cg.cc:107.  std::max(a, b) is (a < b) ? b : a: a NaN p.Ap stays a
// NaN (the comparison is false), a NaN bound is ignored.  fmax would return the other operand in both cases.
__device__ __forceinline__ double safeguarded_alpha(double rsold, double conj)
{
    const double bound = rsold * kNearZero;
    return rsold / ((conj < bound) ? bound : conj);
}


// ------------------------------------------------------------------------------------------------
// reductions: fixed order => bitwise reproducible for a given launch shape
// ------------------------------------------------------------------------------------------------

// Sums of R independent per-lane values over the 64 lanes at once (R a power of two).  Instead of R butterflies of six
// exchanges each, the lanes first split the rows among themselves: at every halving step a lane keeps half of its rows
// and hands the other half to its partner, so the exchanges go R/2 + R/4 + ... + 1, and the rest of the butterfly runs
// on ONE value.  R = 8: 10 exchanges instead of 48.  Afterwards v[0] of lane L is the total of row L >> (6 - log2 R)
// (every lane of that group holds it).  Fixed order => bitwise reproducible for a given shape.
// v + (v of the partner lane), the partner given by a DPP control word: no LDS crossbar, a few cycles instead of a
// ds_bpermute round trip.  0xB1 / 0x4E: quad_perm = lane ^ 1 / lane ^ 2.  0x141 / 0x140: row_half_mirror / row_mirror
// pair lane i with 7 - i of its 8 / 15 - i of its 16 lanes -- as good as lane ^ 4 / lane ^ 8 for a sum once the lower
// levels have made the lanes of each quad / each 8 hold the same value (which is the order they are used in below).
template <int CTRL>
__device__ __forceinline__ double dpp_add(double v)
{
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xF, 0xF, false);
    return v + __hiloint2double(hi, lo);
}

// Total of one value over groups of SPAN consecutive lanes (SPAN a power of two <= 64), every lane of the group gets it:
// levels 1, 2, 4, 8 by DPP, 16 and 32 by ds_bpermute.
template <int SPAN>
__device__ __forceinline__ double group_sum(double v)
{
    if constexpr (SPAN > 32) v += __shfl_xor(v, 32, 64);
    if constexpr (SPAN > 16) v += __shfl_xor(v, 16, 64);
    if constexpr (SPAN > 1) v = dpp_add<0xB1>(v);
    if constexpr (SPAN > 2) v = dpp_add<0x4E>(v);
    if constexpr (SPAN > 4) v = dpp_add<0x141>(v);
    if constexpr (SPAN > 8) v = dpp_add<0x140>(v);
    return v;
}

__device__ __forceinline__ double wave_sum(double v)
{
    return group_sum<64>(v);   // every lane holds the total
}

template <int R, int N, int WIDTH>
__device__ __forceinline__ void wave_sum_rows_step(double (&v)[R], int lane)
{
    if constexpr (N > 1) {
        const bool upper = (lane & WIDTH) != 0;
#pragma unroll
        for (int i = 0; i < N / 2; ++i) {
            const double send = upper ? v[i] : v[i + N / 2];
            const double keep = upper ? v[i + N / 2] : v[i];
            v[i] = keep + __shfl_xor(send, WIDTH, 64);
        }
        wave_sum_rows_step<R, N / 2, WIDTH / 2>(v, lane);
    } else {
        v[0] = group_sum<2 * WIDTH>(v[0]);   // the lanes that still differ: groups of 2*WIDTH = 64/R
    }
}

template <int R>
__device__ __forceinline__ int wave_sum_rows(double (&v)[R], int lane)
{
    static_assert(R >= 1 && R <= 64 && (R & (R - 1)) == 0, "rows per workgroup must be a power of two");
    wave_sum_rows_step<R, R, 32>(v, lane);
    return lane / (64 / R);   // the row this lane holds: its top log2(R) lane bits
}

template <int WAVES>
__device__ __forceinline__ double block_sum(double v, double *lds /* >= WAVES doubles */)
{
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();   // protect lds against a previous use
    if (lane == 0) lds[w] = v;
    __syncthreads();
    double s = lds[0];
#pragma unroll
    for (int i = 1; i < WAVES; ++i) s += lds[i];
    return s;
}

// ------------------------------------------------------------------------------------------------
// p.Ap = sum of every K1 workgroup partial of every rank (cblas_ddot + MPI_Allreduce, cg.cc:105-106): the thread's share, to be
// finished by block_sum<4>.  Every workgroup of every rank (K3 in all its forms, the low-rank, multi-right-hand-side and
// multi-shift updates) folds the same partials in the same fixed order: bit-identical everywhere.  The partials of rank q are
// the `count` doubles at tails + q * S; one contiguous run is nranks == 1.  All 256 threads of the workgroup (tid: the thread's index among
// them, where a workgroup runs several such groups: cgx_multi_pc.hip).
// ------------------------------------------------------------------------------------------------
// One row per thread (k_update_xr): one flat index over (rank, partial).  With a few partials per rank (the chunk partials of a
// multi-GPU run: n/512 in all) every thread has at most one or two loads, all in flight together -- a loop over the ranks with
// one load each was a chain of P dependent round trips (5.9 us at P = 8 against 4.8 at P = 2 and 4, round 3).
__device__ __forceinline__ double fold_pap(const double *tails, int nranks, int S, int count, int tid = threadIdx.x)
{
    const int total = nranks * count;
    auto at = [&](int f) {
        if (nranks == 1) return tails[f];
        const int q = f / count;
        return tails[(long)q * S + (f - q * count)];
    };
    double cs = 0.0;
    for (int f = tid; f < total; f += 4 * 256) {           // four independent loads in flight (clamped, not branched around)
        double a[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int g = f + u * 256;
            const double val = at(g < total ? g : total - 1);
            a[u] = g < total ? val : 0.0;
        }
        cs += (a[0] + a[1]) + (a[2] + a[3]);
    }
    return cs;
}

// Rows strided over the workgroups (k_update_xr_strided): a lane-strided sum, rank by rank.
__device__ __forceinline__ double fold_pap_strided(const double *tails, int nranks, int S, int count)
{
    double cs = 0.0;
    for (int q = 0; q < nranks; ++q) {
        const double *tail = tails + (long)q * S;
        for (int j = threadIdx.x; j < count; j += 256) cs += tail[j];
    }
    return cs;
}

// The tag of an epoch: 1 + (epoch mod (2^32 - 1)), i.e. 1 ... 2^32 - 1, never 0; consecutive epochs of one parity (e-2, e)
// always differ, and two epochs share a tag only 2^32 - 1 apart.
__device__ __forceinline__ unsigned p2p_tag(unsigned long long epoch)
{
    return (unsigned)(epoch % 0xFFFFFFFFull) + 1u;
}
// Both words of one double leave as ONE 16-byte store with the system-scope write-through bits (what the two relaxed 8-byte
// atomic stores of the definition compile to, `global_store_dwordx2 ... sc0 sc1`, as one instruction and one request: over
// xGMI a request is a packet, and 8-byte packets cost 2.7x the time per byte of 16-byte ones, measured for sc1 stores in the
// guide).  Nothing depends on the two words arriving together: each validates itself.
typedef unsigned u4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void tagged_store(unsigned long long *dst, double v, unsigned tag)
{
    const unsigned long long bits = (unsigned long long)__double_as_longlong(v);
    const u4 w = {(unsigned)bits, tag, (unsigned)(bits >> 32), tag};   // little endian: {lo32 | tag<<32}, {hi32 | tag<<32}
    asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1" : : "v"(dst), "v"(w) : "memory");
}


// One entry of generate_lap2d_matrix, cg.cc:178-185 (0 <= i, j < size).
__device__ __forceinline__ double lap2d_entry(int size, int inc, long i, long j)
{
    if (j == i) return 4.0;                                      // cg.cc:183
    if (i > 0 && j == i - 1) return -1.0;                        // cg.cc:182
    if (i < size - 1 && j == i + 1) return -1.0;                 // cg.cc:184
    if (i > inc && j == i - 1 - inc) return -1.0;                // cg.cc:181
    if (i < size - 1 - inc && j == i + 1 + inc) return -1.0;     // cg.cc:185
    return 0.0;                                                  // cg.cc:178-180
}

// ------------------------------------------------------------------------------------------------
// shared by the per-launch GEMV kernels (cgx_kernels.hip: K1; cgx_symv.hip: the symmetric form)
// ------------------------------------------------------------------------------------------------
template <bool NT>
__device__ __forceinline__ d2 load_a(const double *ptr)
{
    if constexpr (NT) return __builtin_nontemporal_load(reinterpret_cast<const d2 *>(ptr));
    else return *reinterpret_cast<const d2 *>(ptr);
}

// ------------------------------------------------------------------------------------------------
// the exchanged residual (SegView) and the scalar sums over ranks
// ------------------------------------------------------------------------------------------------
// Owner of column c: q = min(c / n_loc, nranks-1), without an integer division: the host supplies the
// round-up magic number (div_magic, div_shift) for n_loc (seg_finalize), exact for 0 <= c < 2^31.
__device__ __forceinline__ int seg_owner(const SegView &sv, int c)
{
    if (sv.n_loc <= 0) return sv.nranks - 1;   // N < P: floor(N/P) = 0 rows everywhere but on the last rank (cg.cc:255-266)
    const int t = (sv.div_shift == 32) ? c : (int)(__umulhi((unsigned)c, sv.div_magic) >> sv.div_shift);
    return t < sv.nranks - 1 ? t : sv.nranks - 1;
}

__device__ __forceinline__ double seg_load(const SegView &sv, int c)   // r[c], c < n
{
    const int q = (sv.nranks > 1) ? seg_owner(sv, c) : 0;
    return sv.base[c + q * sv.seg_gap];   // q*S + (c - q*n_loc)
}

__device__ __forceinline__ double seg_sum_slot(const SegView &sv, int slot)
{
    double s = sv.base[sv.Sr + slot];
    for (int q = 1; q < sv.nranks; ++q) s += sv.base[(long)q * sv.S + sv.Sr + slot];   // rank order
    return s;
}

// gathered layout on every shard: [rank q][slot v], kSlots doubles per rank
__device__ __forceinline__ double sum_ranks(const double *__restrict__ gathered, int slot, int nranks)
{
    double s = gathered[slot];
    for (int q = 1; q < nranks; ++q) s += gathered[q * kSlots + slot];   // rank order, same on every shard
    return s;
}

// Tail of iteration k-1, evaluated redundantly (and identically) by every WAVE of K1(k).
// r.r = fixed-order fold of K3's per-workgroup partials (the tail of the replicated-r segment): every wave of every
// workgroup of every rank folds the same values the same way (lane-strided sums, then the shuffle butterfly), so the
// break decision is the same everywhere, and no in-kernel grid reduction (ticket + fences, ~4 us at the end of K3) is
// needed.  No LDS and no workgroup barrier: on gfx9 a barrier's release fence drains vmcnt, i.e. it would wait for every
// A load a kernel has already issued ahead of the head.  The head is cut in two so that a kernel can put its first
// A loads between the halves: head_issue sends out the head's own loads (done, rsold, up to 256 partials), head_finish
// consumes them -- loads return in order, so the wait in between covers the head's loads only.
struct IterHead {
    double beta;
    bool stop;
};

struct HeadLoads {
    double rsold;
    int done;
    double a[4];
};

__device__ __forceinline__ HeadLoads head_issue(const Scalars *sc, const SegView &sv, int k)
{
    HeadLoads hl;
    const int nparts = sv.S - sv.Sr, lane = threadIdx.x & 63;
    const double *part = sv.base + sv.Sr;
    hl.done = sc->done;                                  // converged earlier: the whole grid drains immediately
    hl.rsold = sc->rs[(k > 0 ? k - 1 : 0) & 1];          // stored by the previous K1: independent of the fold
    // unconditional loads (clamped index, value discarded by a select): a load behind a branch would make the number of
    // loads in flight path dependent, and the compiler then waits for ALL of them (vmcnt(0)) instead of counting
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int t = lane + 64 * u;
        const double val = part[t < nparts ? t : nparts - 1];
        hl.a[u] = (t < nparts) ? val : 0.0;
    }
    return hl;
}

__device__ __forceinline__ IterHead head_finish(const HeadLoads &hl, Scalars *sc, const SegView &sv, int k, double tol)
{
    IterHead h{0.0, false};
    const int nparts = sv.S - sv.Sr, lane = threadIdx.x & 63;
    const double *part = sv.base + sv.Sr;
    double v = (hl.a[0] + hl.a[1]) + (hl.a[2] + hl.a[3]);
    for (int t = lane + 256; t < nparts; t += 256) {     // more than 256 partials: n > 65536
        const double a0 = part[t], a1 = (t + 64 < nparts) ? part[t + 64] : 0.0;
        const double a2 = (t + 128 < nparts) ? part[t + 128] : 0.0, a3 = (t + 192 < nparts) ? part[t + 192] : 0.0;
        v += (a0 + a1) + (a2 + a3);
    }
    const double rsnew = wave_sum(v);                                // r.r over all rows, cg.cc:116-117 (k==0: cg.cc:91-92)
    const bool first = (blockIdx.x == 0 && threadIdx.x == 0) && !hl.done;   // nothing is written once converged
    if (k == 0) {                                                    // p = r (cg.cc:85): beta = 0, p_old = 0
        if (first) { sc->rs[0] = rsnew; sc->rs[1] = rsnew; }
        return h;
    }
    if (first) sc->rs[k & 1] = rsnew;                                // rsold = rsnew, cg.cc:132
    if (sqrt(rsnew) < tol) {                                         // cg.cc:120-121: break before the p update
        if (first) { sc->k_final = k - 1; sc->done = 1; }
        h.stop = true;
        return h;
    }
    h.beta = rsnew / hl.rsold;                                       // cg.cc:124
    return h;
}

// Both halves back to back; *done = the flag as loaded.  All lanes of the wave must be active (shuffles).
__device__ __forceinline__ IterHead iteration_head(Scalars *sc, const SegView &sv, int k, double tol, int *done)
{
    const HeadLoads hl = head_issue(sc, sv, k);
    *done = hl.done;
    return head_finish(hl, sc, sv, k, tol);
}

// ---- the Jacobi (PRECOND) form of the head ----------------------------------------------------------
// sv is the replicated z = D^-1 r: [z (lda) | r.z partials | r.r partials], both partial sets S - Sr long, in the update
// kernel's workgroup order.  Both sets are folded in the same fixed order as the plain head's one set: rho = r.z gives beta,
// r.r the break; rs[] holds rho, rr[] holds r.r.  Same rule as above: all loads issued before the first wait, unconditionally.
struct HeadLoadsPc {
    double rsold;
    int done;
    double a[4];   // r.z partials
    double b[4];   // r.r partials
};

__device__ __forceinline__ HeadLoadsPc head_issue_pc(const Scalars *sc, const SegView &sv, int k)
{
    HeadLoadsPc hl;
    const int nparts = sv.S - sv.Sr, lane = threadIdx.x & 63;
    const double *pz = sv.base + sv.Sr, *pr = sv.base + sv.S;
    hl.done = sc->done;
    hl.rsold = sc->rs[(k > 0 ? k - 1 : 0) & 1];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int t = lane + 64 * u, tc = t < nparts ? t : nparts - 1;
        const double vz = pz[tc], vr = pr[tc];
        hl.a[u] = (t < nparts) ? vz : 0.0;
        hl.b[u] = (t < nparts) ? vr : 0.0;
    }
    return hl;
}

__device__ __forceinline__ IterHead head_finish_pc(const HeadLoadsPc &hl, Scalars *sc, const SegView &sv, int k, double tol)
{
    IterHead h{0.0, false};
    const int nparts = sv.S - sv.Sr, lane = threadIdx.x & 63;
    const double *pz = sv.base + sv.Sr, *pr = sv.base + sv.S;
    double vz = (hl.a[0] + hl.a[1]) + (hl.a[2] + hl.a[3]);
    double vr = (hl.b[0] + hl.b[1]) + (hl.b[2] + hl.b[3]);
    for (int t = lane + 256; t < nparts; t += 256) {                // more than 256 partials: n > 65536
        double az[4], ar[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const bool ok = t + 64 * u < nparts;
            az[u] = ok ? pz[t + 64 * u] : 0.0;
            ar[u] = ok ? pr[t + 64 * u] : 0.0;
        }
        vz += (az[0] + az[1]) + (az[2] + az[3]);
        vr += (ar[0] + ar[1]) + (ar[2] + ar[3]);
    }
    const double rznew = wave_sum(vz);                               // rho_k = r.z
    const double rrnew = wave_sum(vr);                               // r.r: the stopping test and the report
    const bool first = (blockIdx.x == 0 && threadIdx.x == 0) && !hl.done;
    if (k == 0) {                                                    // p = z: beta = 0, p_old = 0
        if (first) { sc->rs[0] = rznew; sc->rs[1] = rznew; sc->rr[0] = rrnew; sc->rr[1] = rrnew; }
        return h;
    }
    if (first) { sc->rs[k & 1] = rznew; sc->rr[k & 1] = rrnew; }
    if (sqrt(rrnew) < tol) {                                         // tol bounds the true recursive residual, as without Jacobi
        if (first) { sc->k_final = k - 1; sc->done = 1; }
        h.stop = true;
        return h;
    }
    h.beta = rznew / hl.rsold;
    return h;
}

// The head of either form, chosen at compile time: the K1 families take PRE as a template parameter.
template <bool PRE>
using HeadLoadsOf = typename std::conditional<PRE, HeadLoadsPc, HeadLoads>::type;

template <bool PRE>
__device__ __forceinline__ HeadLoadsOf<PRE> head_issue_t(const Scalars *sc, const SegView &sv, int k)
{
    if constexpr (PRE) return head_issue_pc(sc, sv, k);
    else return head_issue(sc, sv, k);
}

template <bool PRE>
__device__ __forceinline__ IterHead head_finish_t(const HeadLoadsOf<PRE> &hl, Scalars *sc, const SegView &sv, int k, double tol)
{
    if constexpr (PRE) return head_finish_pc(hl, sc, sv, k, tol);
    else return head_finish(hl, sc, sv, k, tol);
}

template <bool PRE>
__device__ __forceinline__ IterHead iteration_head_t(Scalars *sc, const SegView &sv, int k, double tol, int *done)
{
    const HeadLoadsOf<PRE> hl = head_issue_t<PRE>(sc, sv, k);
    *done = hl.done;
    return head_finish_t<PRE>(hl, sc, sv, k, tol);
}

// One row of the Jacobi update, the same function wherever z = dinv r is formed -- the Jacobi kind of K3's three bodies
// (update_xr_tile, update_xr_strided, init_residual_rows in cgx_kernels.hip: k_update_xr_pc, k_update_xr_strided_pc,
// k_init_residual_pc) and k_pcg_update_p2p -- so that every transport produces the same bits: r_new = r - alpha Ap,
// z = dinv r_new, and the row's terms of r.r and r.z.  (The block kind fills the same PcRow from its chain: bj_row.)
struct PcRow {
    double r, z, rr, rz;
};
__device__ __forceinline__ PcRow pc_row(double r_new, double dinv_i)
{
    PcRow o;
    o.r = r_new;
    o.z = dinv_i * r_new;
    o.rr = r_new * r_new;
    o.rz = r_new * o.z;
    return o;
}
__device__ __forceinline__ PcRow pc_update_row(double alpha, double ap_i, double r_i, double dinv_i)
{
    return pc_row(fma(-alpha, ap_i, r_i), dinv_i);
}
// the workgroup's two partials: r.z in z's tail, r.r behind it
__device__ __forceinline__ void pc_store_partials(const SegView &zv, int wg, double rz, double rr)
{
    zv.base[zv.Sr + wg] = rz;
    zv.base[zv.S + wg] = rr;
}

// ------------------------------------------------------------------------------------------------
// shared by the multi-vector K1 of cgx_multi.hip and cgx_multi_pc.hip (its body: cgx_multi_gemv.inc)
// ------------------------------------------------------------------------------------------------
constexpr int kMultiWaves = 8;
constexpr int kMultiThreads = kMultiWaves * 64;
constexpr int kMultiChunk = 256;                     // columns staged per chunk (2 steps of 128)
constexpr int kMultiSteps = kMultiChunk / 128;

// rows per wave for a kernel width: R * W <= 32 partial sums per lane; W = 16 takes one row (two spill: the staged P and the
// unrolled LDS reads of 16 columns come on top of the sums)
template <int W>
struct MultiShape {
    static constexpr int R = W <= 4 ? 8 : (W == 8 ? 4 : 1);
};

// Per column j: the head of iteration k (cg.cc:116-132 of iteration k-1) from the r.r partials rrp[j * g3 + 0 .. g3) -- PRE: and
// the r.z partials rzp[j * g3 + 0 .. g3).  Run by one wave; every workgroup of the launch folds the same values in the same
// order, so every workgroup takes the same decision.  Writes (workgroup 0 only, and nothing for a column that is already
// frozen): rs (PRE: rho = r.z there, r.r in mp->rr), done, k_final.  Returns whether the column runs this iteration, and its beta.
template <bool PRE>
__device__ __forceinline__ bool multi_head(MultiScalars *ms, MultiPcScalars *mp, const double *__restrict__ rzp,
                                           const double *__restrict__ rrp, int g3, int j, int k, double tol, bool writer,
                                           double *beta)
{
    const int lane = threadIdx.x & 63;
    const int done = ms->done[j];
    const double rsold = ms->rs[j][(k > 0 ? k - 1 : 0) & 1];
    const double *part = rrp + (long)j * g3;
    if constexpr (!PRE) {
        double v = 0.0;
        for (int t = lane; t < g3; t += 256) {
            double a[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int f = t + 64 * u;
                const double val = part[f < g3 ? f : g3 - 1];
                a[u] = f < g3 ? val : 0.0;
            }
            v += (a[0] + a[1]) + (a[2] + a[3]);
        }
        const double rsnew = wave_sum(v);                       // r.r, cg.cc:116-117 (k == 0: cg.cc:91-92)
        *beta = 0.0;
        if (done) return false;                                 // frozen: nothing is written any more
        const bool first = writer && lane == 0;
        if (k == 0) {                                           // p = r (cg.cc:85): beta = 0, p_old = 0
            if (first) { ms->rs[j][0] = rsnew; ms->rs[j][1] = rsnew; }
            return true;
        }
        if (first) ms->rs[j][k & 1] = rsnew;                    // rsold = rsnew, cg.cc:132
        if (sqrt(rsnew) < tol) {                                // cg.cc:120-121: break before the p update
            if (first) { ms->k_final[j] = k - 1; ms->done[j] = 1; }
            return false;
        }
        *beta = rsnew / rsold;                                  // cg.cc:124
        return true;
    } else {
        const double *partz = rzp + (long)j * g3;
        double v = 0.0, vz = 0.0;
        for (int t = lane; t < g3; t += 256) {
            double a[4], z[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int f = t + 64 * u, fc = f < g3 ? f : g3 - 1;
                const double val = part[fc], valz = partz[fc];
                a[u] = f < g3 ? val : 0.0;
                z[u] = f < g3 ? valz : 0.0;
            }
            v += (a[0] + a[1]) + (a[2] + a[3]);
            vz += (z[0] + z[1]) + (z[2] + z[3]);
        }
        const double rrnew = wave_sum(v);                       // r.r: the break and the report
        const double rho = wave_sum(vz);                        // r.z: beta, and alpha's numerator in the update kernel
        *beta = 0.0;
        if (done) return false;
        const bool first = writer && lane == 0;
        if (k == 0) {                                           // p = z: beta = 0, p_old = 0
            if (first) { ms->rs[j][0] = rho; ms->rs[j][1] = rho; mp->rr[j][0] = rrnew; mp->rr[j][1] = rrnew; }
            return true;
        }
        if (first) { ms->rs[j][k & 1] = rho; mp->rr[j][k & 1] = rrnew; }
        if (sqrt(rrnew) < tol) {                                // tol bounds the recursive residual, as without a preconditioner
            if (first) { ms->k_final[j] = k - 1; ms->done[j] = 1; }
            return false;
        }
        *beta = rho / rsold;
        return true;
    }
}


// p_new for the column pair (c, c+1); pad columns (>= n) stay exactly 0.
// SINGLE (one shard): r is contiguous and zero padded up to lda, one 16-B load.
template <bool SINGLE>
__device__ __forceinline__ d2 make_p(const SegView &sv, double beta, d2 p_old, int c)
{
    d2 r;
    if constexpr (SINGLE) {
        r = *reinterpret_cast<const d2 *>(sv.base + c);
    } else {
        r.x = (c < sv.n) ? seg_load(sv, c) : 0.0;
        r.y = (c + 1 < sv.n) ? seg_load(sv, c + 1) : 0.0;
    }
    d2 p;
    p.x = fma(beta, p_old.x, r.x);                                   // cg.cc:127-129
    p.y = fma(beta, p_old.y, r.y);
    return p;
}

// ------------------------------------------------------------------------------------------------
// the chunk arithmetic of the multi-rank exchange ("Chunks" in cgx_kernels.hip): k_prefold_ap and the pushers of the
// fused P2P update (cgx_p2p.hip) call the same functions, so every transport ships the same bits
// ------------------------------------------------------------------------------------------------
// Branch-free: every load is unconditional (clamped index, value dropped by a select), so that all of them -- up to
// kMaxSplit pieces and the two elements of p -- are in flight together; loads behind a branch or in a loop of unknown
// length are waited for one by one (seen in the ISA: s_waitcnt vmcnt(0) after each piece).
constexpr int kMaxSplit = 8;
__device__ __forceinline__ d2 chunk_pair(const double *__restrict__ parts, int split, long stride, int row, int Sr)
{
    const int rc = row < Sr ? row : Sr - 2;                           // Sr is even and >= 2, slices are 16-B aligned
    d2 v[kMaxSplit];
#pragma unroll
    for (int sp = 0; sp < kMaxSplit; ++sp)
        v[sp] = *reinterpret_cast<const d2 *>(parts + (sp < split ? sp : split - 1) * stride + rc);
    d2 a = v[0];
#pragma unroll
    for (int sp = 1; sp < kMaxSplit; ++sp) {                          // ascending piece order
        a.x = sp < split ? a.x + v[sp].x : a.x;
        a.y = sp < split ? a.y + v[sp].y : a.y;
    }
    if (row >= Sr) a = d2{0.0, 0.0};
    return a;
}

// the pair's two elements of p_sub (p_loc = p_new + row0; row0 may be odd: 8-B loads), 0 behind the last row
__device__ __forceinline__ d2 chunk_p(const double *__restrict__ p_loc, int row, int rows)
{
    const int last = rows > 0 ? rows - 1 : 0;                         // rows == 0: p_loc[0] is still inside p (zero pad)
    const double p0 = p_loc[row < rows ? row : last];
    const double p1 = p_loc[row + 1 < rows ? row + 1 : last];
    return d2{row < rows ? p0 : 0.0, row + 1 < rows ? p1 : 0.0};
}

template <int WAVES>
__device__ __forceinline__ double chunk_dot(d2 p, d2 a, double *lds)
{
    return block_sum<WAVES>(fma(p.y, a.y, p.x * a.x), lds);
}

}  // namespace cgx
