// cgx_internal.h -- what the translation units of libcgx share: the context, the per-shard buffers, the error
// macros and the internal helpers.  Nothing here is part of the C ABI (include/cgx.h).
#pragma once

#include "../../include/cgx.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <functional>
#include <string>
#include <vector>

#include "cgx_kernels.h"
#include "cgx_rccl.h"
#include "cgx_tridiag.h"

namespace cgxi {

using cgx::Scalars;

struct Shard {
    int rank = 0;
    int row0 = 0;
    int rows = 0;
    double *A = nullptr;         // rows x lda, row-major, pad columns zero (CGX_MATRIX_DENSE)
    double *dia_vals = nullptr;  // CGX_MATRIX_BANDED: ndiag x dia.ld, the non-zero diagonals of the row block
    cgx::DiaView dia{};
    long long *csr_rp = nullptr; // CGX_MATRIX_CSR: row pointers (rows + 1, local: csr_rp[0] = 0), global columns, values
    int *csr_col = nullptr;
    double *csr_vals = nullptr;
    cgx::CsrView csr{};
    double *b_full = nullptr;    // n doubles: b is replicated like r (the reference builds the full b on every rank, cg.cc:218-234)
    // One GPU, dense storage (where the persistent kernels of cgx_resident.hip / cgx_stream.hip may run the loop): x, rbuf, p[1] and
    // sc are carved out of ONE block of solver state (cgx::state_off_*), and there are two such blocks -- a persistent launch
    // reads state[cur] and writes state[cur ^ 1], and only a launch that came back clean makes the written block the current one
    // (bind_state).  Every other configuration allocates the four buffers one by one and state[] stays null.
    double *state[2] = {nullptr, nullptr};
    int cur = 0;
    double *x = nullptr;         // rows
    double *p[2] = {nullptr, nullptr};   // lda doubles each: the replicated p (cg.cc:57), ping-pong over iterations
    double *apg = nullptr;       // nranks * S doubles: exchanged segments [Ap slice | p.Ap partials] (cgx::SegView apv)
    double *rbuf = nullptr;      // lda + kSlots doubles: the replicated r and its scalars (cgx::SegView rv, one segment)
    double *ap_parts = nullptr;  // plan.split > 1: split x seg_Sr doubles, the column pieces of the fused K1's Ap
    double *k1_scratch = nullptr;   // chunked exchange: where K1's per-workgroup p.Ap partials go (only the gemv probe reads them;
                                    // the segment tail then holds one partial per chunk of the slice instead)
    double *partials = nullptr;  // scratch: per-workgroup partial sums of K3 and of the setup kernels
    double *sym_parts = nullptr; // plan variant 6 (exactly symmetric A, cgx_symv.hip): nb x lda doubles, the tile kernel's slots
    size_t sym_parts_bytes = 0;
    Scalars *sc = nullptr;
    double *gathered = nullptr;  // kMaxRanks * kSlots doubles (DEBUG scalars of all ranks)
    cgx::GemvPlan plan{};
    cgx::SegView apv{}, rv{};
    // Jacobi, made at the first preconditioned solve of a problem: the replicated inverse diagonal (lda
    // doubles, zero padded) and the replicated z = D^-1 r laid out as rbuf with a second partial set behind the first
    // ([z | r.z partials | r.r partials], cgx::SegView zv: rv's geometry)
    double *dinv = nullptr;
    double *zbuf = nullptr;
    // block Jacobi: the replicated block inverses, W[t * lda + i] = (D_b^-1)(i, s(i) + t); w_block x lda
    // doubles, made at the first solve with cgx_set_preconditioner_block > 1, remade when the block size changes
    double *W = nullptr;
    int w_block = 0;
    cgx::SegView zv{};
    int npartials = 0;
    double *Ap() const { return apg + (size_t)rank * apv.S; }          // this shard's Ap slice (K1 output)
    double *tail() const { return Ap() + apv.Sr; }                      // this shard's segment tail: the p.Ap partials that travel
    double *k1_part() const { return k1_scratch ? k1_scratch : tail(); }   // K1's per-workgroup p.Ap partials
};


}  // namespace cgxi

struct cgx_ctx {
    cgx_config cfg{};
    int device = 0;
    hipStream_t stream = nullptr;
    int nranks = 1;
    int m = 0, n = 0;
    long lda = 0;
    int max_iter = 0;
    double tol = 1e-10;   // m_tolerance, code/MPI/cg.hh:56
    std::vector<int> start_rows, num_rows;
    std::vector<cgxi::Shard> shards;   // 1 (SELF / RCCL) or nranks (LOOPBACK)
    std::vector<double> b_host;
    bool have_matrix = false, have_b = false;
    bool banded = false;         // cfg.matrix_format == CGX_MATRIX_BANDED (opt-in, not the reference's storage)
    bool csr = false;            // cfg.matrix_format == CGX_MATRIX_CSR (opt-in)
    bool sparse() const { return banded || csr; }   // the storages whose K1 keeps its own partials (no dense-only paths)
    int precond = CGX_PRECOND_NONE;   // cgx_set_preconditioner: read by cgx_solve_begin, fixed until cgx_solve_end
    int precond_block = 1;       // cgx_set_preconditioner_block: 1 = point Jacobi (dinv), > 1 = block Jacobi (W); read at begin
    bool dinv_valid = false;     // every shard's dinv (block 1) / W (block > 1) holds the checked inverse of the current matrix's
                                 // diagonal (blocks) for precond_block: lowered behind every writer of A and by a new block size
    int *d_jbad = nullptr;       // device word: first row of a diagonal entry Jacobi cannot take (set-up only)
    // CGX_PRECOND_PIVCHOL (one GPU, dense): the settings belong to the context, the factor to the problem
    int precond_rank = 32;       // cgx_set_preconditioner_rank: columns of L, read at begin
    double precond_shift = 0.0;  // cgx_set_preconditioner_shift: 0 = the mean remaining diagonal
    bool lr_valid = false;       // L, C^-1 and delta hold the factor of the current matrix for precond_rank / precond_shift: lowered
                                 // behind every writer of A (beside dinv_valid) and by a new rank or shift
    double lr_delta = 0.0;       // the shift in use, read back behind the set-up
    double *lr_L = nullptr;      // lr_L_rank x lda doubles, column-major at the matrix pitch
    int lr_L_rank = 0;
    double *lr_block = nullptr;  // the set-up's and the loop's work space (cgx::LrWork, carved by lr_work)
    size_t lr_block_bytes = 0;
    bool res_parked = false;     // the persistent kernel would take this problem, but the preconditioner keeps it on the per-launch path

    // RCCL
    const cgx::RcclApi *rccl = nullptr;
    ncclComm_t comm = nullptr;
    // direct peer exchange (CGX_COMM_P2P)
    unsigned char *mailbox = nullptr;        // own fine-grained mailbox
    size_t mailbox_bytes = 0;
    bool mailbox_on_host = false;            // test only (cgx_probe_p2p_mailbox_to_host): the mailbox lives in pinned host memory
    // test only (cgx_probe_p2p_host_mailboxes): EVERY rank's mailbox is a POSIX shared-memory segment registered with the
    // runtime; host_maps[q] = this process's mapping of rank q's segment (own included), nullptr otherwise
    bool mailbox_shm = false;
    std::string shm_prefix;
    void *host_maps[cgx::kMaxRanks] = {nullptr};
    bool p2p_ready = false;                  // peers' mailboxes are mapped
    cgx::MailboxView mv{};
    unsigned long long p2p_epoch[cgx::kP2pChannels] = {0, 0, 0};
    int *d_p2p_err = nullptr;                // device word set when a bounded wait expired
    long long p2p_timeout_ticks = 0;         // 100 MHz wall-clock ticks

    int seg_S = 0, seg_Sr = 0;   // exchange segment geometry (equal for all ranks)
    int npart = 0;               // p.Ap partials per rank in the segment tail: K1's workgroups (max grid over ranks), or, chunked,
                                 // the chunks of a slice (cgx::chunks_per_rank(seg_Sr))
    bool chunked = false;        // the tail holds one partial per chunk (cgx_kernels.hip "Chunks"): every multi-rank dense
                                 // run and every fused P2P update; else K1's own partials (one GPU; banded storage)
    int resident_limit = 0;      // > 0: test override of the co-residency bound of the fused P2P update (cgx_probe_set_resident_limit)

    // the persistent kernels (cgx_resident.hip: n <= 4096, A on the chip; cgx_stream.hip: n <= 16384, A streamed): one GPU, dense
    int cus = 0;                             // compute units of the device
    size_t lds_per_cu = 0;                   // LDS bytes a workgroup can be given
    bool resident = false;                   // the current problem runs the loop as one persistent kernel
    cgx::ResidentPlan rplan{};
    unsigned long long *res_xbuf = nullptr;  // exchange buffer of the resident kernel's workgroups (tagged words)
    size_t res_xbuf_bytes = 0;
    unsigned long long res_epoch = 0;        // epochs handed out so far (monotonic over the life of the context)
    int *d_res_err = nullptr;                // device word raised when a wait inside the resident kernel expired
    long long res_timeout_ticks = 0;
    int res_lock_fd = -1;                    // advisory lock file of the device: one resident grid at a time (see resident_steps)
    bool res_lock_gave_up = false;           // a wait for that lock ran into its bound once: later launches do not wait again
    int res_mute_wg = -1;                    // test only (cgx_probe_resident_test): workgroup that skips its first publish, next launch
    bool res_forced = false;                 // gemv_variant 40000: a launch whose waits expire is an error, not a fallback
    cgx::ResidentTail *h_res_tail = nullptr; // pinned: what a persistent launch reports (written by the kernel itself, cgx_kernels.h)
    unsigned res_stamp = 0;                  // the number of the most recent persistent launch (never 0 once one has run)
    long long res_rec[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // the waits of the current solve's launches, summed up (cgx_get_resident_record)
    bool lean = false;                       // the solve under way began with the one-kernel set-up (zero initial guess, persistent kernel)
    bool oneshot = false;                    // cgx_solve is running begin / steps / end in one go: the end may be enqueued behind the loop
    bool end_enqueued = false;               // ... and has been (verification GEMV + end kernel are behind the persistent launch, h_stage is filled)
    long long res_fallbacks = 0;             // persistent launches of this context whose waits expired and that were redone on the per-launch path

    // loopback pointer tables (device)
    double **d_gathered_ptrs = nullptr;
    cgx::Scalars **d_scalar_ptrs = nullptr;

    // solve state
    bool in_solve = false;
    int k = 0;              // iterations enqueued so far
    bool done = false;
    int k_final = 0;
    int *h_flags = nullptr;   // pinned: 2 polling slots + 1 for read_flags_sync, each {done, k_final}
    double *h_stage = nullptr;   // pinned, n + 16 doubles: x0 in / x out go through it, so that solve() never waits for the
                                 // runtime's first-use set-up of pageable copies (8 ms inside the reference's timing
                                 // window, measured); nullptr above 8 Mi rows (then the copies are direct)
    hipEvent_t flag_ev[2] = {nullptr, nullptr};
    double t_begin = 0, t_loop = 0;

    // K1 timing
    std::vector<hipEvent_t> ev_pool;
    size_t ev_used = 0;
    double gemv_ms_sum = 0, gemv_ms_min = 0, gemv_ms_max = 0;
    long long gemv_launches = 0, gemv_discarded = 0;
    long long gemv_seq = 0;              // K1 launches of the current cgx_solve_steps call
    std::vector<float> gemv_samples;     // their durations (ms), most recent steps call
    bool gemv_timed_last = false;        // the most recent K1 launch was event-timed (the update kernel of that iteration follows suit)
    std::vector<hipEvent_t> upd_pool;    // cfg.profile_update: event pairs around the update kernels of the timed iterations
    size_t upd_used = 0;
    std::vector<float> upd_samples;      // their durations (ms), most recent steps call
    hipEvent_t steps_ev[2] = {nullptr, nullptr};   // markers around the kernels of the most recent steps call (profiling on)
    bool steps_ev_pending = false;
    double steps_device_ms = 0;

    // several right-hand sides (cgx_solve_multi, cgx_multi_host.cpp): ONE device block holding kMaxRhs-wide B, X, R, P[2], Y and the
    // partials and scalars of the multi kernels, apart from the single path's buffers; made on first use, freed with the problem
    double *multi = nullptr;
    size_t multi_bytes = 0;
    // ... and what cgx_solve_multi_pc needs on top (Z, the r.z partials, the partials of L^T r, r.r's scalars): a block of its own,
    // made on the first preconditioned multi call and freed with the problem, so that the plain block keeps its layout
    double *multi_pc = nullptr;
    size_t multi_pc_bytes = 0;
    // multi-shift CG (cgx_solve_shifted, cgx_shift_host.cpp): ONE device block holding the kMaxShifts-wide x and p of the shifts, the
    // block of the final verification and the shift scalars; made on first use, freed with the problem
    double *shift = nullptr;
    size_t shift_bytes = 0;
    // MINRES (cgx_solve_minres, cgx_minres_host.cpp): ONE device block holding the kMaxMinresShifts-wide x and the two direction
    // blocks of the shifts, the block of the final verification, the two recurrence vectors, the partials and the scalars; made on
    // first use, freed with the problem
    double *minres = nullptr;
    size_t minres_bytes = 0;
    // Lanczos quadrature (cgx_lanczos, cgx_trace_slq, cgx_lanczos_host.cpp): ONE device block holding the two kMaxRhs-wide vector
    // blocks of the recurrence, Y, the partials, the alpha / beta histories and the scalars; made on first use, freed with the problem
    double *lanczos = nullptr;
    size_t lanczos_bytes = 0;
    // ... and the preconditioned recurrence's own block (cgx_lanczos_pc, cgx_trace_slq_pc, cgx_lanczos_pc_host.cpp): w, v_prev, u, Y,
    // the partials (K1m's, two w.u sets, those of L^T w), the histories and the scalars; made on first use, freed with the problem
    double *lanczos_pc = nullptr;
    size_t lanczos_pc_bytes = 0;
    // matrix functions (cgx_apply_function, cgx_funm_host.cpp): the coefficient table, the step counts, the result block and the kept
    // Lanczos basis (steps x nvec x lda doubles of the call); made on first use, made again when a call needs more, freed with
    // the problem
    double *funm = nullptr;
    size_t funm_bytes = 0;
    // extreme eigenpairs (cgx_eigenpairs, cgx_eigs_host.cpp): the work vectors, partials, histories, the Ritz-vector block and the
    // reorthogonalised basis ((steps + 1) x lda doubles of the call); made on first use, made again when a call needs more, freed
    // with the problem
    double *eigs = nullptr;
    size_t eigs_bytes = 0;

    int fault_after = -1;     // >= 0: HIP_TRY calls left until one is made to fail (cgx_probe_set_fault_after, error-path tests only)

    std::string err;
};


namespace cgxi {

extern thread_local std::string g_create_error;   // error of the last failed cgx_create on this thread

double wall_now();
cgx_status fail(cgx_ctx *ctx, cgx_status st, const std::string &msg);

// Fault injection for the error-path tests (tools/leak_check.py, tests): after cgx_probe_set_fault_after(ctx, N) the
// (N+1)-th HIP call of the context made through HIP_TRY is not made and reports hipErrorUnknown instead.  Only the explicit
// probe call arms it: nothing in a user's environment can make a production call fail.
inline bool fault_due(cgx_ctx *ctx)
{
    if (!ctx || ctx->fault_after < 0) return false;
    if (ctx->fault_after == 0) { ctx->fault_after = -1; return true; }
    --ctx->fault_after;
    return false;
}

// An early return must not leave work of this context in flight: several entry points enqueue asynchronous copies into
// their own locals (a result struct on the stack, a scratch vector) and synchronise further down; if a call in between --
// or, under fault injection, the synchronisation itself -- fails, the copy would land in memory that is gone.  So the
// failure path drains the context's stream first (best effort; the error that is reported is the original one).
inline void quiesce(cgx_ctx *ctx)
{
    if (ctx && ctx->stream) (void)hipStreamSynchronize(ctx->stream);
}

#define HIP_TRY(ctx, call)                                                                              \
    do {                                                                                                \
        hipError_t e_ = cgxi::fault_due(ctx) ? hipErrorUnknown : (call);                                \
        if (e_ != hipSuccess) {                                                                         \
            cgx_status st_ = (e_ == hipErrorOutOfMemory) ? CGX_ERR_OOM                                  \
                             : (e_ == hipErrorNoDevice || e_ == hipErrorInvalidDevice) ? CGX_ERR_NO_DEVICE \
                                                                                       : CGX_ERR_HIP;   \
            cgxi::quiesce(ctx);                                                                         \
            return fail(ctx, st_, std::string(#call) + ": " + hipGetErrorString(e_));                   \
        }                                                                                               \
    } while (0)

#define NCCL_TRY(ctx, call)                                                                             \
    do {                                                                                                \
        ncclResult_t r_ = (call);                                                                       \
        if (r_ != ncclSuccess) {                                                                        \
            cgxi::quiesce(ctx);                                                                         \
            return fail(ctx, CGX_ERR_RCCL, std::string(#call) + ": " + (ctx)->rccl->GetErrorString(r_)); \
        }                                                                                               \
    } while (0)

#define CGX_TRY(call)                      \
    do {                                   \
        cgx_status s_ = (call);            \
        if (s_ != CGX_OK) return s_;       \
    } while (0)


// Device allocations and events of ONE function: released on every return path (hipFree waits for the device, so work
// still queued on a buffer when an error return unwinds is finished first).
struct DeviceScratch {
    std::vector<void *> ptrs;
    std::vector<hipEvent_t> events;
    DeviceScratch() = default;
    DeviceScratch(const DeviceScratch &) = delete;
    DeviceScratch &operator=(const DeviceScratch &) = delete;
    ~DeviceScratch()
    {
        for (void *p : ptrs) (void)hipFree(p);
        for (hipEvent_t e : events) (void)hipEventDestroy(e);
    }
    template <class T>
    hipError_t alloc(T **out, size_t bytes)
    {
        void *p = nullptr;
        const hipError_t e = hipMalloc(&p, bytes);
        if (e == hipSuccess) ptrs.push_back(p);
        *out = static_cast<T *>(p);
        return e;
    }
    hipError_t event(hipEvent_t *out)
    {
        const hipError_t e = hipEventCreate(out);
        if (e == hipSuccess) events.push_back(*out);
        return e;
    }
};

// cgx_context.cpp
void partition_rows(int N, int psize, int *start_rows, int *num_rows);
void free_problem(cgx_ctx *ctx);
void bind_state(cgxi::Shard &s, long lda);     // point x / rbuf / p[1] / sc (and rv.base) into state[cur]
long p2p_fixed_prefix(int nranks);
cgx_status setup_problem(cgx_ctx *ctx, int n);       // allocate the shards of an n x n problem (contents: caller)
// Behind every writer of A: where the symmetric K1 could run (one shard, dense, n > kSymvMinN, the default plan) A is checked for
// exact symmetry on the device, and the plan becomes variant 6 or the general K1 accordingly (both ways).
cgx_status plan_symmetric(cgx_ctx *ctx);

int configured_variant(const cgx_ctx *ctx);   // cfg.gemv_variant, or CGX_GEMV_VARIANT where that is <= 0

// cgx_matrix.cpp
cgx_status alloc_dia(cgx_ctx *ctx, Shard &s, const std::vector<int> &offs);
// CGX_MATRIX_CSR: (re)allocate shard s for nnz entries (row pointers zeroed), and the K1 plan once every shard is filled
cgx_status alloc_csr(cgx_ctx *ctx, Shard &s, long long nnz);
void plan_csr_shards(cgx_ctx *ctx);
// A Matrix-Market coordinate file as MatrixCOO::read leaves it (matrix_coo.cc:7-60): sizes, symmetry, 0-based entries in
// file order.  Host only; parsed on `nthreads` threads.
struct MtxEntries {
    int m = 0, n = 0, nz = 0;
    bool sym = false;
    std::vector<int> I, J;
    std::vector<double> a;
};
cgx_status parse_matrix_market(const char *path, MtxEntries *out, std::string *err, int nthreads, bool header_only = false);
int default_parse_threads();   // CGX_MTX_THREADS, else the host's hardware threads, at most 16

// cgx_precond.cpp
cgx_status prepare_jacobi(cgx_ctx *ctx);   // inside cgx_solve_begin: refusals, buffers, and once per matrix dinv or the block inverses
cgx_status prepare_lowrank(cgx_ctx *ctx);  // the same for CGX_PRECOND_PIVCHOL: once per matrix, rank and shift the factor
cgx::LrWork lr_work(const cgx_ctx *ctx);   // the pieces of ctx->lr_block (null pointers before the first prepare_lowrank)
// What the multi-column kernels take of the context's preconditioner (Jacobi or pivoted Cholesky, behind prepare_multi_precond);
// tpart: the caller's own room for the partials of L^T r, kMaxRhs x lr_grid(n) x kLrLd doubles
cgx::PcFactor pc_factor(const cgx_ctx *ctx, double *tpart);
// The preconditioner of a multi-vector call (cgx_solve_multi_pc, the preconditioned Lanczos calls), behind the argument checks: the
// refusals of the single path's set-up with their status and message, block Jacobi refused, and -- once per matrix (rank, shift) --
// the inverse diagonal or the factor, by the two functions above.
cgx_status prepare_multi_precond(cgx_ctx *ctx, const std::string &fn);

// cgx_solve.cpp: the exchanges, one iteration, the persistent launches
cgx_status p2p_allgather(cgx_ctx *ctx, int chan, const double *src, int count, double *dst, long dst_stride, int copy_self,
                         int tail_off = 0, int tail_n = 0, int sum_off = 0);
cgx_status gather_scalars(cgx_ctx *ctx);
cgx_status gather_segments(cgx_ctx *ctx, bool with_tail);
cgx_status run_gemv_plain(cgx_ctx *ctx, Shard &s, const double *v_full);
cgx_status enqueue_iteration(cgx_ctx *ctx, int k);          // one body of the loop cg.cc:96-137: K1 fused, the exchange, K3
cgx_status check_p2p_error(cgx_ctx *ctx);
cgx_status resident_steps(cgx_ctx *ctx, int nsteps, int *redo);
// cgx_solve.cpp: what cgx_solve_steps / _end, cgx_solve_multi and cgx_solve_shifted share (and run_polled below)
void reset_gemv_stats(cgx_ctx *ctx);
// The timing decision of the next K1 launch of a steps call: an event pair to bracket it with, or two nulls.
cgx_status next_gemv_events(cgx_ctx *ctx, hipEvent_t *e0, hipEvent_t *e1);
cgx_status harvest_gemv_events(cgx_ctx *ctx);              // fold the recorded pairs into the K1 statistics (after a sync)
void fill_k1_stats(const cgx_ctx *ctx, cgx_result *res);   // launches, avg / min / max / median, discarded, steps_device_ms
double one_gpu_gemv_bytes(const cgx_ctx *ctx);             // algorithmic bytes of one K1 launch of shard 0: dense, CSR or banded
// The refusals every one-GPU entry point begins with, in this order: no context (no message), no problem, an open begin / end
// pair, more than one GPU.
cgx_status check_one_gpu_call(cgx_ctx *ctx, const std::string &fn);
// A side block of the context (cgx_ctx::multi, cgx_ctx::shift): allocated and zeroed on first use, freed again if that fails.
cgx_status ensure_side_block(cgx_ctx *ctx, double **block, size_t *block_bytes, size_t bytes);

// THE verification of the k-column solves (cgx_solve_multi / _multi_pc / _shifted / _minres), enqueued on the context's stream: the
// true residuals of ncol systems.  X, Y: kMaxRhs x lda blocks (column j at + j * lda); Y_j = A x_j -- dense: one plain K1m pass
// over `width` columns with k1p / ms as its partials and scalar block, CSR: one SpMV per column -- then norms[3 j ...] =
// ||Y_j + sigma_j x_j - b_j||^2, ||b_j||^2, ||x_j||^2 (launch_column_norms: b_j = b + j * ldb; sigma: host array, or nullptr).
cgx_status column_residual_norms(cgx_ctx *ctx, int ncol, int width, const double *X, double *Y, double *k1p, cgx::MultiScalars *ms,
                                 const double *b, long ldb, const double *sigma, double *norms);
// ... and THE filler of their results: one cgx_result per column from the two wall times, gemv_bytes, the K1 statistics (k1_stats;
// else they stay 0), the host copy of those norms (x_norm, rel_residual) and what only the solve knows of column j.
struct ColumnOutcome {
    int iterations, converged;
    double residual_prev, residual_last;
};
void fill_column_results(const cgx_ctx *ctx, cgx_result *res, int ncol, double t_begin, double t_loop, double gemv_bytes, bool k1_stats,
                         const double (*norms)[3], const std::function<ColumnOutcome(int)> &outcome);
// The refusals of cgx_solve_shifted and cgx_solve_minres in the order check_multi (cgx_multi_host.cpp) makes them: context, problem,
// transport and storage, arguments.  limit: the name of the bound on nshift; negative_ok: shifts of either sign; precond / form:
// what the message about a preconditioner says, and which form the persistent kernels lack.
cgx_status check_shift_call(cgx_ctx *ctx, const char *name, const char *limit, bool negative_ok, const char *precond, const char *form,
                            int nshift, const double *sigma, const double *X, long ldx);

// ... and one that grows (cgx_ctx::funm, cgx_ctx::eigs): made on first use, made again when a call needs more than it holds.
// detail: what the out-of-memory message says the bytes are for.
cgx_status ensure_growing_block(cgx_ctx *ctx, double **block, size_t *block_bytes, size_t bytes, const std::string &fn,
                                const std::string &detail);
// check_one_gpu_call, then dense storage
cgx_status check_dense_one_gpu(cgx_ctx *ctx, const std::string &fn);

// host rows (one vector per row, pitch ld) <-> a device block (column j at + j * lda); rows 0 .. n-1 only
inline cgx_status upload_columns(cgx_ctx *ctx, double *dst, const double *src, long ld, size_t ncol)
{
    HIP_TRY(ctx, hipMemcpy2DAsync(dst, (size_t)ctx->lda * sizeof(double), src, (size_t)ld * sizeof(double),
                                  (size_t)ctx->n * sizeof(double), ncol, hipMemcpyHostToDevice, ctx->stream));
    return CGX_OK;
}

inline cgx_status download_columns(cgx_ctx *ctx, double *dst, long ld, const double *src, size_t ncol)
{
    HIP_TRY(ctx, hipMemcpy2DAsync(dst, (size_t)ld * sizeof(double), src, (size_t)ctx->lda * sizeof(double),
                                  (size_t)ctx->n * sizeof(double), ncol, hipMemcpyDeviceToHost, ctx->stream));
    return CGX_OK;
}

// What the plain multi-vector K1 (launch_multi_gemv, fused = false) takes on one GPU: Y = A v for nrhs columns and the v.Av partials
inline cgx::MultiArgs plain_k1m_args(const cgx_ctx *ctx, int nrhs, const double *v, double *Y, double *partials)
{
    cgx::MultiArgs g{};
    g.A = ctx->shards[0].A;
    g.lda = ctx->lda;
    g.n = ctx->n;
    g.nrhs = nrhs;
    g.v = v;
    g.Y = Y;
    g.partials = partials;
    return g;
}

// cgx_lanczos_host.cpp: what the Lanczos family shares (DESIGN.md sections 17 - 20)
cgx_status check_lanczos_steps(cgx_ctx *ctx, const std::string &fn, int steps);
// check_dense_one_gpu, "a preconditioner is set and would be ignored", check_lanczos_steps: every call on the plain recurrence
cgx_status check_lanczos(cgx_ctx *ctx, const std::string &fn, int steps);
// The side block of a recurrence: cgx_ctx::lanczos, or, pc, cgx_ctx::lanczos_pc, which alone has the pieces U and tpart.
struct LanczosView {
    double *V[2], *U, *Y;           // kMaxRhs x lda each (column j at + j * lda): w / v_prev in ping-pong, u = M^-1 w, K1m's product
    double *k1p;                    // kMaxRhs x k1p_stride(n): K1m's partials
    double *wwp[2];                 // kMaxRhs x multi_update_grid(n) each: the ||w||^2 (pc: w.u) partials, ping-pong over the steps
    double *tpart;                  // kMaxRhs x lr_grid(n) x kLrLd: the partials of L^T w (pivoted Cholesky)
    double *alpha, *beta;           // kMaxRhs x kMaxLanczosSteps each: the histories
    cgx::LanczosScalars *ls;
};
cgx_status lanczos_block(cgx_ctx *ctx, bool pc, LanczosView *v);   // made on first use
// THE recurrence: nvec start vectors through `steps` steps, plain or, pc, with the context's prepared preconditioner.  V0 (one
// vector per row, pitch ldv) is uploaded, or, V0 == nullptr, the block V[0] is taken as the caller left it on the device.  alpha,
// beta: nvec rows of `steps` doubles, zero at t >= m[j]; z2[j] = ||V0_j||^2 (pc: eta0^2 = V0_j . M^-1 V0_j) as the device summed
// it.  col0: the number of row 0 in the caller's own count, for the message about a bad start vector.  basis != nullptr
// (cgx_apply_function): behind step t the block that now holds the normalised v_t is copied into slot t, nvec * lda doubles each.
cgx_status lanczos_run(cgx_ctx *ctx, const std::string &fn, bool pc, int nvec, int steps, const double *V0, long ldv, int col0,
                       double *alpha, double *beta, int *m, double *z2, double *basis = nullptr);
// THE stochastic Lanczos quadrature on that recurrence: the mean over nprobe probes of z2 sum_i weight_i f(theta_i), its standard
// error, the values per probe and the extreme Ritz values (the last two may be null).  The probes are the rows of Z, or, Z == nullptr,
// what device_probes(probe0, nb) leaves in V[0] of the recurrence's block, or, without one, the library's Rademacher signs of `seed`
// made on the host.
using SlqProbes = std::function<cgx_status(int probe0, int nb)>;
cgx_status check_slq_args(cgx_ctx *ctx, const std::string &fn, int fn_kind, int nprobe, const double *estimate, const double *std_error,
                          const double *Z, long ldz);
cgx_status slq_estimate(cgx_ctx *ctx, const std::string &fn, bool pc, int fn_kind, int nprobe, int steps, unsigned long long seed,
                        const double *Z, long ldz, const SlqProbes &device_probes, double *estimate, double *std_error, double *per_probe,
                        double *ritz);

// Lays a side block out in 128-byte aligned pieces; base == nullptr only measures (bytes()).
struct Carver {
    double *base;
    size_t off = 0;
    double *take(size_t count)
    {
        double *p = base ? base + off : nullptr;
        off += (count + 15) / 16 * 16;
        return p;
    }
    template <class T>
    T *take_struct() { return reinterpret_cast<T *>(take((sizeof(T) + 7) / 8)); }
    size_t bytes() const { return off * sizeof(double); }
};

// p.Ap partials per column that any multi-vector K1 launch may write: the largest K1m grid over the widths
inline int k1p_stride(int n)
{
    int g = 0;
    for (int w = 1; w <= cgx::kMaxRhs; w *= 2) g = std::max(g, cgx::multi_gemv_grid(n, w));
    return g;
}

// THE polled host loop of every solve on the per-launch kernels: up to `count` calls of enqueue_one(i), i = 0, 1, ..., in batches
// of cfg.check_every (made positive by cgx_create).  Behind each batch the two flag words at d_flags ({done, k_final} or their
// like) are copied into a pinned slot and an event is recorded; then the host waits for the batch BEFORE it, so one batch stays
// queued, and stops at a raised first word.  window: markers on the stream in front of the first and behind the last kernel
// (steps_ev, read by harvest_gemv_events).  *enqueued: the iterations of the batches that were enqueued completely.  The body is
// a template parameter so that it is inlined: at small n this loop is the host's hot path.
template <class Body>
cgx_status run_polled(cgx_ctx *ctx, const int *d_flags, int count, bool window, Body &&enqueue_one, int *enqueued)
{
    hipStream_t st = ctx->stream;
    *enqueued = 0;
    if (window) {
        for (auto &e : ctx->steps_ev)
            if (!e) HIP_TRY(ctx, hipEventCreate(&e));
        HIP_TRY(ctx, hipEventRecord(ctx->steps_ev[0], st));
    }
    const int every = ctx->cfg.check_every;
    int k = 0, slot = 0;
    bool pending[2] = {false, false}, stop = false;
    while (k < count && !stop) {
        const int batch = std::min(count - k, every);
        for (int i = 0; i < batch; ++i) CGX_TRY(enqueue_one(k + i));
        k += batch;
        *enqueued = k;
        HIP_TRY(ctx, hipMemcpyAsync(ctx->h_flags + 2 * slot, d_flags, 2 * sizeof(int), hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipEventRecord(ctx->flag_ev[slot], st));
        pending[slot] = true;
        slot ^= 1;
        if (pending[slot]) {
            HIP_TRY(ctx, hipEventSynchronize(ctx->flag_ev[slot]));
            pending[slot] = false;
            if (ctx->h_flags[2 * slot]) stop = true;   // identical on every rank: rsnew is bit-identical (cg.cc:117-121)
        }
    }
    if (window) {   // (a stop marker is only ever paired with the start marker of the same call)
        HIP_TRY(ctx, hipEventRecord(ctx->steps_ev[1], st));
        ctx->steps_ev_pending = true;
    }
    return CGX_OK;
}

}  // namespace cgxi
