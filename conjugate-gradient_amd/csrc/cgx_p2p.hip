// cgx_p2p.hip -- the direct peer exchange (CGX_COMM_P2P) of the multi-rank CG loop, on gfx950.
//
// Two kernels.  k_mailbox_allgather is a lean all-gather over the IPC-mapped mailboxes (set-up, verification and the
// separate-exchange path).  k_update_xr_p2p is K3 (cgx_kernels.hip) with the iteration's exchange inside it: the prefold of
// K1's Ap pieces, the hand-over of [Ap slice | p.Ap partials] to every peer, and the update of x and r, in one launch.  The
// chunk arithmetic (chunk_pair / chunk_p / chunk_dot) is shared with k_prefold_ap through cgx_device.h: every transport gives
// the same bits.
#include "cgx_kernels.h"
#include "cgx_device.h"

#include <hip/hip_ext.h>

namespace cgx {

// ------------------------------------------------------------------------------------------------
// Direct peer exchange over xGMI: replaces one RCCL all-gather launch.
// Protocol per (channel, epoch), placement independent:
//   producer: plain 16-B stores of the payload into the PEER's mailbox slot [epoch&1][my rank]; every storing
//             thread fences at system scope; workgroup barrier; one lane stores flag = epoch with a system-scope
//             release atomic into the peer's flag word [channel][my rank];
//   consumer: one lane polls its OWN flag word [channel][peer] with system-scope acquire loads (bounded by the
//             100 MHz wall clock), workgroup barrier, every thread fences (acquire, system) and reads the slot
//             with system-scope loads (never served from a stale cache line), then plain-stores into the
//             ordinary working buffer the next kernel reads.
// Two parities suffice: a rank can start epoch e+2 only after every peer delivered e+1, which a peer does only
// after the kernel that consumed epoch e on that peer has finished (stream order).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_mailbox_allgather(MailboxView mv, int chan, unsigned long long epoch,
                                                            const double *__restrict__ src, int count, int tail_off,
                                                            int tail_n, double *__restrict__ dst, long dst_stride,
                                                            int sum_off, int copy_self, long long timeout_ticks, int *err)
{
    const int peer = blockIdx.x;
    const int tid = threadIdx.x;
    // an earlier wait expired: do not wait again, let the host see it.  Decided per workgroup (another workgroup may
    // raise the word while this one starts), so that no thread is left alone at a barrier.
    if (__syncthreads_or(__hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) return;
    __shared__ double lds[4];
    double tail_sum = 0.0;
    if (tail_n > 0) {
        // fold my tail (the K1 partials) in a fixed order and ship ONE double behind the main payload (every
        // workgroup computes the same bits): the local half of MPI_Allreduce (cg.cc:106) rides in the exchange
        double v = 0.0;
        for (int i = tid; i < tail_n; i += 256) v += src[tail_off + i];
        tail_sum = block_sum<4>(v, lds);
    }
    if (peer == mv.rank) {
        if (copy_self)
            for (int i = tid; i < count; i += 256) dst[(long)mv.rank * dst_stride + i] = src[i];
        if (tail_n > 0 && tid == 0) dst[(long)mv.rank * dst_stride + sum_off] = tail_sum;
        return;
    }
    const int parity = (int)(epoch & 1);
    const long slot = mv.slot_bytes[chan];
    // ---- push my contribution into the peer's mailbox: [count doubles | tail sum] ----------------------------
    {
        double *out = reinterpret_cast<double *>(mv.base[peer] + mv.data_off[chan] +
                                                 ((long)parity * mv.nranks + mv.rank) * slot);
        const int pairs = count >> 1;
        for (int i = tid; i < pairs; i += 256)
            *reinterpret_cast<d2 *>(out + 2 * i) = *reinterpret_cast<const d2 *>(src + 2 * i);
        if ((count & 1) && tid == 0) out[count - 1] = src[count - 1];
        if (tail_n > 0 && tid == 0) out[count] = tail_sum;
        __threadfence_system();   // every storing wave: write back, wait for its own stores (vmcnt is per wave), before the barrier
        __syncthreads();
        if (tid == 0) {
            unsigned long long *flag = reinterpret_cast<unsigned long long *>(
                mv.base[peer] + ((long)chan * kMaxRanks + mv.rank) * kP2pFlagStride);
            // the same tail as chunk_publish: release fence, its own wait (the compiler drops the one behind buffer_wbl2 when it
            // can prove this wave has nothing outstanding -- harmless here, every wave has drained above, but not left to that),
            // then the flag as a relaxed system-scope store
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __hip_atomic_store(flag, epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
    // ---- wait for the peer's contribution in MY mailbox, then copy it out ------------------------------------
    __shared__ int s_ok;
    if (tid == 0) {
        const unsigned long long *flag = reinterpret_cast<const unsigned long long *>(
            mv.base[mv.rank] + ((long)chan * kMaxRanks + peer) * kP2pFlagStride);
        const long long t0 = wall_clock64();
        int ok = 1;
        while (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) < epoch) {   // relaxed polls, ONE acquire after
            __builtin_amdgcn_s_sleep(8);
            if (wall_clock64() - t0 > timeout_ticks) {   // every spin is bounded: give up, tell the host
                ok = 0;
                atomicExch(err, 1);
                break;
            }
        }
        s_ok = ok;
    }
    __syncthreads();
    if (!s_ok) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");   // system scope
    {
        const unsigned long long *in = reinterpret_cast<const unsigned long long *>(
            mv.base[mv.rank] + mv.data_off[chan] + ((long)parity * mv.nranks + peer) * slot);
        double *out = dst + (long)peer * dst_stride;
        const int total = count + (tail_n > 0 ? 1 : 0);
        // 8 independent loads in flight per thread: the slot is read straight from memory, never from a cache
        for (int base = 0; base < total; base += 8 * 256) {
            unsigned long long v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int i = base + u * 256 + tid;
                v[u] = (i < total) ? __hip_atomic_load(in + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) : 0ull;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int i = base + u * 256 + tid;
                if (i < count) out[i] = __longlong_as_double((long long)v[u]);
                else if (i == count && tail_n > 0) out[sum_off] = __longlong_as_double((long long)v[u]);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// K3 with the exchange inside (CGX_COMM_P2P): iteration = K1 + this kernel, nothing else.
// The (peer, chunk) pairs -- P x cpr of them, about as many as the kernel has workgroups -- are dealt over the grid: a
// workgroup adds K1's column pieces for ONE chunk of kChunkRows rows, reduces the chunk's p.Ap partial, stores
// [chunk of Ap | partial] into ONE peer's mailbox slot (its own included: own rows take the same road as everybody
// else's) and raises that peer's flag word (me, chunk): one pass of independent loads, one 16-B store per thread, one fence,
// one flag.  (Round 2 had P workgroups push a whole slice each: 8 dependent rounds of loads per pusher, and every
// workgroup folded all of the rank's K1 partials -- 4096 with the columns split 8 ways: 13.4 us against 6.7 unsplit.)
// Then EVERY workgroup waits (bounded) for all P x cpr flags in its own mailbox, lane f polling word f, and reads what
// it needs straight from the slots with system-scope loads: the P x cpr partials, folded in one fixed order (bit-identical
// on every rank, MPI_Allreduce cg.cc:106), and per thread the one Ap element of its row.  No copy-out pass, no kernel
// boundary between exchange and update.  All workgroups must be co-resident (the host checks the occupancy): pushers
// never wait before they have pushed, so every flag a workgroup polls is raised by a workgroup that is running.
// ------------------------------------------------------------------------------------------------
// The flag-word half of the exchange as device functions (chunk_fetch serves both forms).
struct ChunkItem {      // one (peer, chunk) pair of this workgroup, loads issued
    int peer, c, row;
    d2 a, pp;
};

__device__ __forceinline__ ChunkItem chunk_fetch(int pr, int cpr, const double *__restrict__ ap_src, int split, long part_stride,
                                                 int Sr, const double *__restrict__ p_loc, int rows)
{
    ChunkItem it;
    it.peer = pr / cpr;
    it.c = pr - it.peer * cpr;
    it.row = (it.c * 256 + (int)threadIdx.x) * 2;                     // this thread's pair of rows of MY slice
    it.pp = chunk_p(p_loc, it.row, rows);
    it.a = chunk_pair(ap_src, split, part_stride, it.row, Sr);
    return it;
}

// [chunk of Ap | its p.Ap partial] into the peer's slot, then the peer's flag word (me, chunk).
// Release, the producer form of the guide (MI355X_MICROARCH.md, "Valid forms"): EVERY storing wave waits for its own stores
// (`s_waitcnt vmcnt(0)`: the counter is per wave, and neither a barrier nor a workgroup-scope release drains it), then the
// workgroup barrier, then lane 0: one system-scope release fence, its own vmcnt(0), and the flag as a relaxed system-scope
// store.  (Round 3 had only the barrier and a release STORE by lane 0: in the ISA waves 1-3 went from their
// global_store_dwordx4 straight to s_barrier, so over xGMI the flag could have passed their part of the chunk -- the
// one-GPU self-test cannot see that; found by review)
__device__ __forceinline__ void chunk_publish(const MailboxView &mv, int chan, unsigned long long epoch, int cpr, int Sr,
                                              const ChunkItem &it, double *lds)
{
    const int P = mv.nranks, me = mv.rank, par = (int)(epoch & 1);
    const double d = chunk_dot<4>(it.pp, it.a, lds);                  // local part of MPI_Allreduce(p.Ap), cg.cc:105-106
    double *out = reinterpret_cast<double *>(mv.base[it.peer] + mv.data_off[chan] + ((long)par * P + me) * mv.slot_bytes[chan]);
    if (it.row < Sr) *reinterpret_cast<d2 *>(out + it.row) = it.a;
    if (threadIdx.x == 0) out[Sr + it.c] = d;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                  // this wave's stores have been acknowledged
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");                 // system scope
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __hip_atomic_store(reinterpret_cast<unsigned long long *>(mv.base[it.peer] + mv.cflag_off) + (me * cpr + it.c), epoch,
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// Lane f waits for flag word f = (source rank, chunk) of MY mailbox (bounded by the 100 MHz wall clock), then ONE
// system-scope acquire per polling wave, drained before the caller's barrier releases the other waves (the consumer form of
// the guide: relaxed polls -> one acquire -> s_waitcnt vmcnt(0) -> barrier -> loads).  Every load of handed-off bytes
// afterwards is a system-scope load as well, so nothing rests on one mechanism alone when the peer's stores arrive over
// xGMI instead of from a process on the same GPU.  Returns 0 in the lanes whose wait expired.
__device__ __forceinline__ int chunk_wait_all(const MailboxView &mv, unsigned long long epoch, int npairs, long long timeout_ticks,
                                              int *err)
{
    int ok = 1;
    const unsigned long long *flags = reinterpret_cast<const unsigned long long *>(mv.base[mv.rank] + mv.cflag_off);
    for (int f = threadIdx.x; f < npairs; f += 256) {
        const long long t0 = wall_clock64();
        // relaxed polls (an acquire per poll would invalidate caches every time round: 2-3x slower per hop)
        while (__hip_atomic_load(flags + f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) < epoch) {
            __builtin_amdgcn_s_sleep(4);
            if (wall_clock64() - t0 > timeout_ticks) {
                ok = 0;
                atomicExch(err, 1);
                break;
            }
        }
    }
    if (mv.acquire && ((int)threadIdx.x & ~63) < npairs) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    return ok;
}

__device__ __forceinline__ const unsigned long long *chunk_slot(const MailboxView &mv, int chan, unsigned long long epoch, int q)
{
    return reinterpret_cast<const unsigned long long *>(mv.base[mv.rank] + mv.data_off[chan]) +
           ((long)(epoch & 1) * mv.nranks + q) * (mv.slot_bytes[chan] / 8);
}

// this thread's share of all ranks' chunk partials, one fixed order (the caller block-reduces)
__device__ __forceinline__ double chunk_read_partials(const MailboxView &mv, int chan, unsigned long long epoch, int cpr, int Sr,
                                                      int npairs)
{
    double cs = 0.0;
    for (int f = threadIdx.x; f < npairs; f += 256) {
        const int q = f / cpr, c = f - q * cpr;
        cs += __longlong_as_double((long long)__hip_atomic_load(chunk_slot(mv, chan, epoch, q) + Sr + c, __ATOMIC_RELAXED,
                                                                  __HIP_MEMORY_SCOPE_SYSTEM));
    }
    return cs;
}

__device__ __forceinline__ double chunk_read_ap(const MailboxView &mv, int chan, unsigned long long epoch, int q, int off)
{
    return __longlong_as_double((long long)__hip_atomic_load(chunk_slot(mv, chan, epoch, q) + off, __ATOMIC_RELAXED,
                                                              __HIP_MEMORY_SCOPE_SYSTEM));
}

// ------------------------------------------------------------------------------------------------
// Tagged words: the exchange without flags and without fences (cfg.p2p_tagged; the transport self-test decides whether a
// node may use it).  Every double travels as two 8-byte words {32 bits of the value | 32 bits of the epoch}, each written
// with ONE relaxed system-scope atomic store and read with relaxed system-scope atomic loads.  A reader that sees the
// epoch in a word knows that the word's other half belongs to the same store (8-byte atomics are single-copy atomic), and
// it needs nothing else: no word depends on the order in which any other word arrives, so there is no release, no flag,
// no acquire, and no barrier between "the data is there" and "use it" -- the chain is store -> (xGMI) -> the poll that
// hits.  A slot still holds the words of epoch e-2 until they are overwritten: the tag is compared for equality.
// What a tagged slot can hold, and why none of it passes for the current epoch (round 4):
//   * zeros -- the mailbox is zero-filled when it is created, and the tagged region is zero-filled again whenever it is laid
//     out anew (a new problem geometry, the self-test): p2p_tag() is never 0;
//   * tagged words of epoch e-2, e-4, ... of the SAME layout -- every position a reader looks at is rewritten in every
//     epoch of its parity, so the newest stale tag is that of e-2, and p2p_tag(e) != p2p_tag(e-2) for every e;
//   * nothing else: the plain-double all-gathers of the set-up and verification phases (k_mailbox_allgather: x0 / x /
//     the initial Ap) have a slot region and an epoch counter of their own in tagged mode (channel 0), so no plain double is
//     ever stored where a tagged reader polls.  (Round 3 shared channel 1 and relied on "no finite double looks like a tag
//     during the first 2^19 epochs of a context".)
// Twice the bytes on the wire (64 KiB per rank at N = 32768): irrelevant for a latency-bound exchange.
// ------------------------------------------------------------------------------------------------
// polls both words until they carry `tag` (bounded by the wall clock); *ok = 0 if the wait expired
__device__ __forceinline__ double tagged_load(const unsigned long long *src, unsigned tag, long long timeout_ticks, int *err, int *ok)
{
    const long long t0 = wall_clock64();
    unsigned long long w0, w1;
    for (;;) {
        w0 = __hip_atomic_load(src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        w1 = __hip_atomic_load(src + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        if ((unsigned)(w0 >> 32) == tag && (unsigned)(w1 >> 32) == tag) break;
        __builtin_amdgcn_s_sleep(2);
        if (wall_clock64() - t0 > timeout_ticks) {
            *ok = 0;
            atomicExch(err, 1);
            break;
        }
    }
    return __longlong_as_double((long long)((w0 & 0xffffffffull) | (w1 << 32)));
}

__device__ __forceinline__ unsigned long long *tagged_slot(const MailboxView &mv, int owner, int chan, unsigned long long epoch, int q)
{
    return reinterpret_cast<unsigned long long *>(mv.base[owner] + mv.data_off[chan] +
                                                  ((long)(epoch & 1) * mv.nranks + q) * mv.slot_bytes[chan]);
}

// The four instantiations of the fused update.  TAGGED: how the bytes are handed over, flag words (chunk_publish /
// chunk_wait_all) or tagged words; both forms deal the same pairs, compute the same chunk arithmetic and fold the partials
// in the same order, so they give the same bits.  SELFTEST: the transport self-test, the gate in front of every P2P run.
// It runs the production kernel of its form up to the fold, then stores what it received instead of updating r and x:
// vals[i] = the Ap element of row i, sums[blockIdx.x] = the folded partials.  It reads neither sc, r nor x (the host
// passes nullptr), and p_new is only the pattern the pushers send.  vals and sums are unused by the production kernels.
// k_pcg_update_p2p: the Jacobi form, the same body with PRE = true (cgx_p2p_update.inc).  It has the
// same parameter list as the others and takes its two extra pointers in the self-test's slots: vals = the replicated z (laid out
// as rv: the r.z partial goes to z[rv.Sr + wg], the r.r partial to z[rv.S + wg]), sums = dinv.  dinv[i] is loaded with the
// row's other operands, and the row update is pc_update_row (cgx_device.h), as in k_update_xr_pc: the same bits.
template <bool TAGGED, bool SELFTEST>
__global__ __launch_bounds__(256) void k_update_xr_p2p(int n, int rows, int row0, const double *__restrict__ p_new,
                                                        SegView apv, int cpr, MailboxView mv, int chan,
                                                        unsigned long long epoch, double *__restrict__ x, SegView rv,
                                                        Scalars *sc, int parity_rs, long long timeout_ticks, int *err,
                                                        const double *__restrict__ ap_src, int split, long part_stride,
                                                        double *__restrict__ vals, double *__restrict__ sums)
{
    constexpr bool PRE = false;
#include "cgx_p2p_update.inc"
}

template <bool TAGGED>
__global__ __launch_bounds__(256) void k_pcg_update_p2p(int n, int rows, int row0, const double *__restrict__ p_new,
                                                        SegView apv, int cpr, MailboxView mv, int chan,
                                                        unsigned long long epoch, double *__restrict__ x, SegView rv,
                                                        Scalars *sc, int parity_rs, long long timeout_ticks, int *err,
                                                        const double *__restrict__ ap_src, int split, long part_stride,
                                                        double *__restrict__ vals, double *__restrict__ sums)
{
    constexpr bool SELFTEST = false;
    constexpr bool PRE = true;
#include "cgx_p2p_update.inc"
}

// ------------------------------------------------------------------------------------------------
// host-side launchers
// ------------------------------------------------------------------------------------------------
hipError_t launch_mailbox_allgather(const MailboxView &mv, int chan, unsigned long long epoch, const double *src,
                                    int count, int tail_off, int tail_n, double *dst, long dst_stride, int sum_off,
                                    int copy_self, long long timeout_ticks, int *err, hipStream_t s)
{
    hipLaunchKernelGGL(k_mailbox_allgather, dim3(mv.nranks), dim3(256), 0, s, mv, chan, epoch, src, count, tail_off, tail_n,
                       dst, dst_stride, sum_off, copy_self, timeout_ticks, err);
    return hipGetLastError();
}

namespace {

using UpdateXrP2p = decltype(&k_update_xr_p2p<false, false>);

UpdateXrP2p update_xr_p2p_kernel(bool tagged, bool selftest, bool jacobi = false)
{
    if (jacobi) return tagged ? k_pcg_update_p2p<true> : k_pcg_update_p2p<false>;
    if (tagged) return selftest ? k_update_xr_p2p<true, true> : k_update_xr_p2p<true, false>;
    return selftest ? k_update_xr_p2p<false, true> : k_update_xr_p2p<false, false>;
}

// Both entry points below: the production update (vals == sums == nullptr) and the self-test (x, rv, sc unused).
hipError_t launch_p2p(bool selftest, int n, int rows, int row0, const double *p_new, SegView apv, int cpr, const MailboxView &mv,
                      int chan, unsigned long long epoch, double *x, SegView rv, Scalars *sc, int parity, long long timeout_ticks,
                      int *err, const double *ap_src, int split, long stride, double *vals, double *sums, hipStream_t s,
                      hipEvent_t e0, hipEvent_t e1, bool jacobi = false)
{
    if (cpr != chunks_per_rank(apv.Sr) || (long)mv.nranks * cpr > kMaxChunkFlags || split < 1 || split > kMaxSplit)
        return hipErrorInvalidValue;
    hipExtLaunchKernelGGL(update_xr_p2p_kernel(mv.tagged, selftest, jacobi), dim3(update_xr_grid(n)), dim3(256), 0, s, e0, e1, 0, n, rows,
                          row0, p_new, apv, cpr, mv, chan, epoch, x, rv, sc, parity, timeout_ticks, err, ap_src, split, stride,
                          vals, sums);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_update_xr_p2p(int n, int rows, int row0, const double *p_new, SegView apv, int cpr,
                                const MailboxView &mv, int chan, unsigned long long epoch, double *x, SegView rv, Scalars *sc,
                                int parity, long long timeout_ticks, int *err, hipStream_t s, const double *ap_src, int split,
                                long stride, hipEvent_t e0, hipEvent_t e1, const double *dinv, SegView zv)
{
    if (dinv && (zv.S != rv.S || zv.Sr != rv.Sr)) return hipErrorInvalidValue;   // z must be laid out as r
    return launch_p2p(false, n, rows, row0, p_new, apv, cpr, mv, chan, epoch, x, rv, sc, parity, timeout_ticks, err, ap_src, split,
                      stride, dinv ? zv.base : nullptr, const_cast<double *>(dinv), s, e0, e1, dinv != nullptr);
}

hipError_t launch_chunk_exchange_selftest(int n, int rows, int row0, const double *p_like, SegView apv, int cpr,
                                          const MailboxView &mv, int chan, unsigned long long epoch, long long timeout_ticks,
                                          int *err, const double *ap_src, int split, long stride, double *vals, double *sums,
                                          hipStream_t s)
{
    return launch_p2p(true, n, rows, row0, p_like, apv, cpr, mv, chan, epoch, nullptr, SegView{}, nullptr, 0, timeout_ticks, err,
                      ap_src, split, stride, vals, sums, s, nullptr, nullptr);
}

hipError_t update_xr_p2p_resident_limit(int device, bool tagged, int *workgroups)
{
    int per_cu = 0, cus = 0;
    hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, update_xr_p2p_kernel(tagged, false), 256, 0);
    if (e != hipSuccess) return e;
    e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
    if (e != hipSuccess) return e;
    *workgroups = per_cu * cus;
    return hipSuccess;
}

}  // namespace cgx
