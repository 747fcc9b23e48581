/*
 * cgx.h -- C ABI of libcgx, the MI355X (gfx950) drop-in for the reference's CGSolver::solve() path.
 *
 * The reference (federicobetti99/Conjugate-Gradient) has no plugin/FFI layer: its seam is the C++
 * class CGSolver (code/MPI/cg.hh:11-57, code/CUDA/cg.hh:13-45) called once from main
 * (code/MPI/cg_main.cc:28-55).  Each entry point below names the reference member it replaces.
 * A host-side `class CGSolver` with the reference's method names, built on this ABI, lives in
 * conjugate-gradient_amd/host/cg.hh; INTEGRATION.md shows the binding a maintainer would add.
 *
 * Conventions
 *   - plain C, no torch / HIP types in any signature; all pointers are HOST pointers;
 *   - every function returns a cgx_status (0 = ok) and never calls exit();
 *   - a context is not thread-safe: one caller thread (the reference is MPI_THREAD_SINGLE,
 *     code/MPI/cg_main.cc:15);
 *   - all floating point is IEEE fp64, indices are int like the reference (code/MPI/matrix.hh:17)
 *     but device offsets are 64-bit.
 *
 * Sharding (code/MPI/cg.cc:59-75, 236-268): the matrix is row-block partitioned over `nranks`
 * shards exactly as partition_matrix does.  CGX_COMM_RCCL = one OS process per GPU (the MPI model),
 * one RCCL AllGather per iteration over xGMI in place of 2 x MPI_Allreduce + MPI_Allgatherv.
 * CGX_COMM_LOOPBACK = `nranks` logical shards on ONE device in one process (same kernels, same
 * collective sequencing, in-process exchange) -- the CI stand-in for a multi-GPU node.
 */
#ifndef CGX_H
#define CGX_H

#ifdef __cplusplus
extern "C" {
#endif

#define CGX_VERSION 1
#define CGX_UNIQUE_ID_BYTES 128
#define CGX_IPC_HANDLE_BYTES 64

typedef enum cgx_status {
    CGX_OK = 0,
    CGX_ERR_BAD_ARG = 1,      /* null pointer, n <= 0, call out of sequence ...            */
    CGX_ERR_IO = 2,           /* file could not be opened / parsed (matrix_coo.cc:14-33)    */
    CGX_ERR_HIP = 3,          /* a HIP runtime call failed                                  */
    CGX_ERR_RCCL = 4,         /* an RCCL call failed or librccl could not be loaded         */
    CGX_ERR_OOM = 5,          /* host or device allocation failed                           */
    CGX_ERR_NO_DEVICE = 6,    /* no gfx950 device visible: the product path has NO CPU fallback */
    CGX_ERR_UNSUPPORTED = 7,  /* e.g. Matrix-Market field/format this reader does not take  */
    CGX_ERR_P2P = 8           /* direct peer exchange: a bounded wait for a peer expired, or IPC mapping failed */
} cgx_status;

typedef enum cgx_comm_mode {
    CGX_COMM_SELF = 0,        /* 1 shard, 1 device, no collectives (psize == 1)             */
    CGX_COMM_LOOPBACK = 1,    /* nranks logical shards on one device, in-process exchange   */
    CGX_COMM_RCCL = 2,        /* this process is shard `rank` of `nranks`, RCCL over xGMI   */
    CGX_COMM_P2P = 3          /* same process model, but the one exchange per iteration stores straight into the
                                 peers' IPC-mapped mailboxes over xGMI, folded into the update kernel (no RCCL at
                                 all); needs cgx_p2p_export / cgx_p2p_import after cgx_create; two forms of handing the
                                 bytes over: payload + flag words (default), or tagged words (cgx_config.p2p_tagged)   */
} cgx_comm_mode;

/* How the row block is held on the device.  DENSE is the reference's contract (Matrix, code/MPI/matrix.hh:7-29:
 * every one of the n*n entries is stored and streamed by the GEMV) and the only format bench.py measures.
 * BANDED is an OPT-IN fast path that is NOT in the reference: the block is held as its non-zero diagonals (at
 * most CGX_MAX_DIAGONALS of them) and K1 becomes a banded mat-vec -- same CG recurrence, same results to rounding,
 * n/ndiag times less matrix traffic (the reference's unused MatrixCOO::mat_vec,
 * code/MPI/matrix_coo.hh:22-34, is the hint).  A matrix with more diagonals is refused with
 * CGX_ERR_UNSUPPORTED, never silently densified.
 * CSR is a second OPT-IN storage, also NOT in the reference and never used by bench.py: a general sparse row block
 * (compressed sparse rows, global column indices) for matrices that are neither small enough to be
 * dense nor banded.  K1 becomes a CSR mat-vec (plan variant 7); K3, every transport and the Jacobi preconditioner are shared.
 * No n x n or rows x n buffer exists at any point of a CSR ingest.  cgx_read_matrix on CSR keeps every position the file
 * assigns, also where the resolved value is exactly 0 (stored as an explicit zero). */
typedef enum cgx_matrix_format {
    CGX_MATRIX_DENSE = 0,
    CGX_MATRIX_BANDED = 1,
    CGX_MATRIX_CSR = 2
} cgx_matrix_format;
#define CGX_MAX_DIAGONALS 64

typedef struct cgx_config {
    int  struct_version;      /* = CGX_VERSION                                              */
    int  comm_mode;           /* cgx_comm_mode                                              */
    int  device;              /* HIP device ordinal this process drives                     */
    int  rank;                /* CGX_COMM_RCCL: this process's shard; else 0                */
    int  nranks;              /* number of row blocks (the reference's psize)               */
    unsigned char unique_id[CGX_UNIQUE_ID_BYTES]; /* CGX_COMM_RCCL: from cgx_comm_unique_id */
    int  gemv_variant;        /* 0 = library default: the per-launch path (K1 + K3 per iteration) with the K1 shape chosen from the
                                 block size -- or, for a dense matrix of n <= 16384 on one GPU (CGX_COMM_SELF), a PERSISTENT kernel:
                                 the whole loop cg.cc:95-137 as ONE launch whose workgroups exchange Ap among themselves.
                                 n <= 4096: every row group of A stays on the chip, in a CU's LDS (n <= 2048) or in its LDS and
                                 registers with a streamed rest (csrc/cgx_resident.hip; 2-6 us per iteration instead of 7-26);
                                 4096 < n <= 16384: the rows are streamed (all but the few that fit beside them), the vectors
                                 stay in registers (csrc/cgx_stream.hip; the default up to n = 10000, where it measures faster:
                                 18 / 71 / 92-95 us per iteration at n = 5120 / 8192 / 9216 instead of 36 / 80 / 104, the solve
                                 at n = 10000 in 71-74 ms instead of 78; CGX_STREAM_MAX
                                 moves that end).  What the default choice rests on, and what happens when it fails:
                                 all workgroups of such a kernel must be resident at once (checked against the runtime's
                                 occupancy when the problem is set; another tenant of the GPU can still break it), and the
                                 exchange rests on an aligned 8-byte half of a 16-byte write-through store being seen untorn
                                 by another CU -- observed on gfx950 / ROCm 7.2, not an architectural guarantee (the same
                                 caveat as p2p_tagged below).  Every wait inside the kernel is bounded (p2p_timeout_ms); a
                                 launch whose wait expires has written nothing of the solver's state, and under the DEFAULT
                                 choice the library redoes it on the per-launch path and stays there for the rest of the
                                 problem: the call returns CGX_OK, cgx_get_gemv_plan then reports the per-launch shape,
                                 cgx_get_resident_record counts the event and cgx_last_error holds a note.
                                 40000 = ask for the persistent kernel: CGX_ERR_UNSUPPORTED where it cannot be had, and an
                                 expired wait is CGX_ERR_HIP (no fallback; the context stays usable for the next problem);
                                 50000 = the same, but the STREAMING persistent kernel whatever the size (1024 <= n <= 16384);
                                 60000 = the per-launch path with its default shape (as -1), but a symmetric A on one GPU
                                 (plan variant 6, n > 16384) walks its tiles on the grid of 4 workgroups per CU instead of one
                                 tile per workgroup: the same kernel and the same bits, kept as the A/B switch for the walk
                                 ("variant 6"); a general A runs the default K1 shape;
                                 -1 = the per-launch path with its default shape, also where a persistent kernel would fit
                                 (as does CGX_RESIDENT=0 in the environment; CGX_STREAM_MAX=n moves the upper end of the
                                 default, 4096 = never stream); v*10000 + R*100 + U*10 + d = an explicit per-launch K1 shape,
                                 see DESIGN.md "K1 variants".  profile_gemv, profile_update and check_every do not apply to
                                 a persistent kernel (there are no K1 launches to time and no polls: gemv_ms_* stay 0). */
    int  lda_pad;             /* extra doubles added to the row pitch (-1 = library default)*/
    int  check_every;         /* iterations between host polls of the device `done` flag (0 = default) */
    int  profile_gemv;        /* n > 0 = bracket every n-th K1 launch with HIP events (at most 2048 per cgx_solve_steps call);
                                 the FIRST launch of a cgx_solve_steps call starts on a drained stream and is never
                                 a sample unless profile_first is set (its event pair also spans the host's launch latency) */
    int  profile_update;      /* 1 = the update kernel of an iteration (K3, or K3 with the exchange inside) is event-timed as well,
                                 on the same launches as K1 (needs profile_gemv > 0): on a multi-GPU run its duration holds the
                                 wait for the peers, i.e. the cost of the exchange (cgx_get_update_samples).  Default 0: a
                                 timed dispatch costs ~5 us of stream time.  (The field was reserved0 before round 3.) */
    int  p2p_mailbox_kib;     /* CGX_COMM_P2P: mailbox size in KiB (0 = 16384)               */
    int  p2p_timeout_ms;      /* CGX_COMM_P2P: bound of every in-kernel wait (0 = 5000)     */
    int  p2p_separate_exchange; /* CGX_COMM_P2P: 1 = exchange in its own kernel between K1 and K3 (default 0: folded into K3) */
    int  matrix_format;       /* cgx_matrix_format; 0 = dense = the reference's storage     */
    int  profile_first;       /* 1 = also sample the first K1 launch of every cgx_solve_steps call (diagnostics only) */
    int  profile_markers;     /* 0 = the event pair is bound to the K1 dispatch itself (kernel begin/end, what rocprofv3 reports);
                                 1 = hipEventRecord markers before and after it (diagnostics only: adds two packets per launch) */
    int  p2p_no_acquire_fence; /* diagnostics only: 1 = leave out the system-scope acquire fence behind the flag wait of the
                                 fused update kernel (for measuring its cost); default 0 = fence on */
    int  p2p_tagged;          /* CGX_COMM_P2P with the exchange folded into the update kernel: 1 = hand the bytes over as tagged
                                 8-byte words (each carries half a double and the epoch and validates itself: no flags, no
                                 fences; the two words of a double leave as one 16-byte write-through store, readers poll with
                                 relaxed 8-byte system-scope atomic loads); 0 = payload stores + release,
                                 flag words, polls + acquire.  Both forms are checked by cgx_p2p_selftest with their own device
                                 code.  The tagged form rests on an aligned 8-byte half of a 16-byte write-through store arriving
                                 untorn at the peer, which no run on more than one GPU has shown yet: the launchers' `auto` uses
                                 the flag form and this one on request only.  (Was reserved[0].) */
} cgx_config;

typedef struct cgx_result {
    int    iterations;        /* k at loop exit, code/MPI/cg.cc:95-137 (index of converging iteration, or max_iter) */
    int    converged;         /* the break at cg.cc:120-121 was taken                       */
    double residual_prev;     /* sqrt(rsold): the "residual" the DEBUG line prints (cg.cc:152-153) */
    double residual_last;     /* sqrt(rsnew) of the last executed iteration                 */
    double x_norm;            /* ||x||             (cg.cc:151)                              */
    double rel_residual;      /* ||Ax-b|| / ||b||  (cg.cc:145-150)                          */
    double seconds_solve;     /* reference timing window: all of solve() (cg_main.cc:53-55) */
    double seconds_loop;      /* the k-loop only                                            */
    double gemv_ms_avg;       /* mean K1 launch duration (HIP events) over the most recent cgx_solve_steps call, 0 if not profiled */
    double gemv_ms_min;
    long long gemv_launches;  /* K1 launches that were event-timed (= samples behind avg / min / median / max) */
    double gemv_bytes;        /* algorithmic bytes of ONE K1 launch on this shard: 8*(rows*n + n + rows); banded: 8*(rows*ndiag + 2*rows);
                                 CSR: 8*nnz + 4*nnz + 8*(rows+1) + 8*rows + 8*n */
    double gemv_ms_median;    /* median of the samples (SURVEY.md section 8d asks for the median) */
    double gemv_ms_max;
    long long gemv_discarded; /* launches deliberately not sampled although profiling was on: the first one after a drained stream */
    double steps_device_ms;   /* the most recent cgx_solve_steps call on the DEVICE's clock: from a marker in front of its first
                                 kernel to one behind its last (0 if profiling is off); the host's wall clock around the same
                                 call additionally holds launch latency and the final synchronisation */
} cgx_result;

typedef struct cgx_ctx cgx_ctx;

/* ---- life cycle -------------------------------------------------------------------------- */
void        cgx_config_init(cgx_config *cfg);                 /* fills defaults (SELF, device 0, 1 rank) */
cgx_status  cgx_comm_unique_id(unsigned char out[CGX_UNIQUE_ID_BYTES]);  /* ncclGetUniqueId; rank 0 calls it, the launcher broadcasts it (replaces MPI_Init, cg_main.cc:15-20) */
cgx_status  cgx_create(cgx_ctx **out, const cgx_config *cfg);
cgx_status  cgx_destroy(cgx_ctx *ctx);
const char *cgx_last_error(const cgx_ctx *ctx);               /* ctx may be NULL: error of the last failed cgx_create on this thread */
const char *cgx_status_string(cgx_status s);

/* What the transport of this context actually spans, for the benchmark record (replaces MPI_Comm_size / MPI_Comm_rank,
 * cg.cc:50-51, as a CHECK: the values come from the transport, not from the configuration):
 *   *ranks_wired  RCCL: ncclCommCount of the communicator; P2P: mailboxes mapped (own + peers) once imported;
 *                 LOOPBACK: logical shards; SELF: 1
 *   *rank_seen    RCCL: ncclCommUserRank; otherwise the configured rank
 *   device_id     PCI bus id of the device this context drives ("0000:05:00.0"), so that a launcher can count the
 *                 distinct GPUs behind its ranks; at least 32 bytes, may be NULL. */
cgx_status  cgx_get_comm_info(cgx_ctx *ctx, int *comm_mode, int *ranks_wired, int *rank_seen, char *device_id);

/* The K1 (GEMV, cg.cc:100-102) launch shape the library planned for local shard `local_shard` of the current problem,
 * for the benchmark record (which kernel ran): out = {variant (1 column-split, 2 LDS-staged p tiles, 3 banded, 4 = the loop
 * runs in the resident persistent kernel, 5 = in the streaming persistent kernel, 6 = symmetric A from its upper triangle), R rows per workgroup (variant 2: per
 * wave), U steps in flight (variant 4 / 5: column steps of 512 / 1024), waves per workgroup, light (1 = the one-round form;
 * variant 4: rows of a workgroup held in registers, 0 up to n = 2048; variant 5: rows per batch of the ring), split (column
 * pieces per row group, tied to the XCDs; variant 5: rows of a workgroup that stay in LDS and registers instead of being streamed), grid (workgroups of one fused launch; variant 4 / 5: of the persistent kernel, all
 * resident at once), ncols (columns swept)}.
 * Variant 6 = one GPU, dense, n > 16384, the default plan and an A that equals its transpose bit for bit (checked on the device
 * behind every writer of A): A p from the upper triangle's B x B tiles (csrc/cgx_symv.hip); then R = B, U = tiles of the longest
 * workgroup run, waves = 4, light = workgroups of the fold kernel (= p.Ap partials), split = nb = ceil(n / B) (slots per row of
 * the partial buffer), grid = workgroups of the tile kernel, ncols as for variant 1.
 * Variant 7 = CSR storage (csrc/cgx_csr.hip): R = L, lanes of a wave64 per row (1 ... 64; default from the mean entries per
 * row, gemv_variant 70000 + L forces it), U = entries in flight per lane, waves = waves per workgroup (4), light = 0, split = 1,
 * grid = workgroups (min(ceil(rows / 64), 2048), striding above that), ncols as for variant 1.  After a persistent launch has been redone on the per-launch path (gemv_variant
 * above) this reports the per-launch shape. */
#define CGX_GEMV_PLAN_INTS 8
cgx_status  cgx_get_gemv_plan(const cgx_ctx *ctx, int local_shard, int out[CGX_GEMV_PLAN_INTS]);

/* What the waits inside the persistent launches of the current (or most recent) solve cost, so that a slow solve can say why:
 * out = {[0] iterations run, [1] polls of the watched word that had to be repeated, [2] gather rounds that had to be repeated,
 * [3] launches -- all four as workgroup 0 saw them --, [4] workgroup 0: 100-MHz wall-clock ticks from its publish of a
 * launch's FIRST iteration until it had all of Ap (a workgroup that was placed late shows here; largest over the launches),
 * [5] workgroup 0: the longest such span of a LATER iteration in which a poll had to be repeated (the exchange itself; 0 =
 * never), [6] / [7] the same two, largest over ALL workgroups, [8] persistent launches of this context, over its whole life,
 * whose waits expired and that were redone on the per-launch path, [9] 1 = the current problem is on a persistent kernel}.
 * Costs no synchronisation: the record comes back with {done, k_final} behind every launch. */
#define CGX_RESIDENT_RECORD_INTS 10
cgx_status  cgx_get_resident_record(const cgx_ctx *ctx, long long out[CGX_RESIDENT_RECORD_INTS]);

/* ---- CGX_COMM_P2P wire-up (replaces MPI_Init's job for the direct-xGMI transport) --------- */
/* export: this rank's mailbox as an IPC handle.  import: all ranks' handles, rank order (nranks * 64 bytes),
 * gathered by the launcher (torch.distributed, MPI_Allgather, pipes ...).  selftest: `rounds` all-gathers of
 * a known pattern, verified on every rank; *ok = 0 on any mismatch or expired wait (then use CGX_COMM_RCCL).
 * The launcher must agree on `ok` across ranks (all-reduce MIN) before anything else is exchanged: every rank must take the
 * same decision.  (That agreement is not what makes the re-layout of the mailbox for a problem safe: a passing self-test
 * ends with an exchange on the scalar channel, after which every peer has finished reading its self-test slots.) */
cgx_status  cgx_p2p_export(cgx_ctx *ctx, unsigned char out[CGX_IPC_HANDLE_BYTES]);
cgx_status  cgx_p2p_import(cgx_ctx *ctx, const unsigned char *handles);
cgx_status  cgx_p2p_selftest(cgx_ctx *ctx, int rounds, int *ok);

/* ---- CGSolver::partition_matrix, code/MPI/cg.cc:236-268 (pure host function) ------------- */
cgx_status  cgx_partition(int n, int psize, int *start_rows, int *num_rows);

/* ---- problem definition ------------------------------------------------------------------ */
/* CGSolver::generate_lap2d_matrix(size), cg.cc:159-188: builds this shard's row block ON DEVICE,
 * sets m = n = max_iter = size (cg.cc:170-172). */
cgx_status  cgx_generate_lap2d_matrix(cgx_ctx *ctx, int size);
/* CGSolver::read_matrix + Matrix::read (cg.cu:307-321, matrix.cc:6-22): caller hands the dense
 * row-major n x n matrix (host, leading dimension lda doubles); the library copies this shard's
 * rows to the device.  Sets m = n, max_iter = n (code/CUDA/cg.cu:236 loops to m_n). */
cgx_status  cgx_set_matrix_dense(cgx_ctx *ctx, const double *A, long lda, int n);
/* MatrixCOO::read + Matrix::read (matrix_coo.cc:7-60, matrix.cc:6-22) done by the library:
 * Matrix-Market `matrix coordinate {real,integer,double} {general,symmetric}` -> device row block,
 * without a dense n*n host staging copy.  Entries are assigned on the device in the file's order (a later
 * entry for the same element wins, a symmetric entry's mirror follows it), exactly as the sequential loop. */
cgx_status  cgx_read_matrix(cgx_ctx *ctx, const char *mtx_path);
/* CGX_MATRIX_CSR only (any other storage: CGX_ERR_UNSUPPORTED): the global n x n matrix as compressed sparse rows in host
 * arrays, 0-based: row_ptr[0] == 0, row_ptr non-decreasing, row_ptr[n] = nnz; the columns of a row strictly ascending and in
 * [0, n).  Each shard copies its own rows; values are stored as given, explicit zeros included.  A null pointer, n <= 0 or a
 * broken rule gives CGX_ERR_BAD_ARG (cgx_last_error names the first bad row) and leaves the context as it was.  Sets m = n,
 * max_iter = n. */
cgx_status  cgx_set_matrix_csr(cgx_ctx *ctx, int n, const long long *row_ptr, const int *col_idx, const double *vals);
/* CGSolver::init_source_term(h), cg.cc:218-234: b evaluated on the HOST with libm sin so it is
 * bit-identical to the reference's, then this shard's slice is uploaded. */
cgx_status  cgx_init_source_term(cgx_ctx *ctx, double h);
cgx_status  cgx_set_source_term(cgx_ctx *ctx, const double *b /* n doubles */);
/* CGSolver::set_max_iter (cg.cc:204-216) and CGSolver::tolerance (cg.hh:39) */
cgx_status  cgx_set_max_iter(cgx_ctx *ctx, int max_iter);
cgx_status  cgx_set_tolerance(cgx_ctx *ctx, double tol);
cgx_status  cgx_get_size(const cgx_ctx *ctx, int *m, int *n);   /* CGSolver::m(), n() */
/* Preconditioner of the per-launch solver.  CGX_PRECOND_JACOBI: z = D^-1 r with D = diag(A), p0 = z0,
 * alpha = r.z / p.Ap, beta = r.z(new) / r.z(old), p = z + beta p.  The stopping test and everything reported keep their meaning:
 * sqrt(r.r) < tol, residual_prev / residual_last = sqrt(r.r).  The setting belongs to the context, survives new matrices and
 * source terms, starts no GPU work, and takes effect at the next cgx_solve / cgx_solve_begin (between begin and end:
 * CGX_ERR_BAD_ARG; every rank of a multi-rank run passes the same kind).  That begin extracts and gathers the diagonal once per
 * matrix; an entry that is not finite and > 0 gives CGX_ERR_BAD_ARG on every rank (row and value in cgx_last_error).  While it
 * is on, the loop runs on the per-launch path (also where the persistent kernels would take the problem); gemv_variant 40000 /
 * 50000, CGX_MATRIX_BANDED and cgx_solve_multi give CGX_ERR_UNSUPPORTED.  Unknown kind: CGX_ERR_BAD_ARG. */
#define CGX_PRECOND_NONE 0
#define CGX_PRECOND_JACOBI 1
cgx_status  cgx_set_preconditioner(cgx_ctx *ctx, int kind);
cgx_status  cgx_get_preconditioner(const cgx_ctx *ctx, int *kind);
/* The block size of CGX_PRECOND_JACOBI: block = 1 (the default) is the point Jacobi above, exactly its
 * kernels and bits; block in {2, 4, 8, 16, 32, 64, 128, 256} is block Jacobi, z = D_b^-1 r with D_b = the block x block diagonal
 * blocks of A as stored, over the global index ranges [j block, min((j+1) block, n)) (shard boundaries do not cut them).
 * z_i is one fma chain over the block's entries in ascending order, so it depends on (i, block) only, not on the shard count or
 * the transport.  Anything else, or a call between cgx_solve_begin and cgx_solve_end: CGX_ERR_BAD_ARG.  The setting belongs to
 * the context, survives new matrices, starts no GPU work, takes effect at the next begin and is used only while the kind is
 * CGX_PRECOND_JACOBI (every rank passes the same block).  That begin extracts, gathers and inverts the blocks on the device once
 * per matrix and block size (from each block's lower triangle, no pivoting); a block that is not positive definite gives
 * CGX_ERR_BAD_ARG on every rank (its first row in cgx_last_error) and leaves the context usable.  The inverses take
 * 8 * block * lda bytes of device memory per shard (lda = the row pitch, >= n): 1 GiB at n = 2^24 with block 8; a failed
 * allocation is CGX_ERR_OOM.  Refused like point Jacobi (banded storage, cgx_solve_multi, gemv_variant 40000 / 50000), and with
 * block > 1 also CGX_COMM_P2P with the exchange folded into the update kernel: CGX_ERR_UNSUPPORTED at cgx_solve_begin
 * (p2p_separate_exchange = 1 is supported). */
cgx_status  cgx_set_preconditioner_block(cgx_ctx *ctx, int block);
cgx_status  cgx_get_preconditioner_block(const cgx_ctx *ctx, int *block);
/* CGX_PRECOND_PIVCHOL: a rank-k partial Cholesky factor with diagonal pivoting plus a shift, A ~ L L^T +
 * delta I, applied through the Woodbury identity: z = (r - L (delta I + L^T L)^-1 L^T r) / delta.  For dense SPD matrices whose
 * diagonal is nearly constant and whose off-diagonal mass is global (kernel / covariance matrices K + sigma^2 I), where Jacobi
 * does nothing.  The recurrence, the stopping test and every reported field are those of CGX_PRECOND_JACOBI above.  One GPU and
 * dense storage: more than one rank or a comm_mode other than CGX_COMM_SELF, CGX_MATRIX_BANDED, CGX_MATRIX_CSR and gemv_variant
 * 40000 / 50000 and a K1 shape with split columns (gemv_variant ending in 3, 4 or 5) give CGX_ERR_UNSUPPORTED at cgx_solve_begin
 * (cgx_solve_multi and cgx_solve_shifted refuse any preconditioner).
 * An enumerator, not a macro: the CGX_PRECOND_* macros are the two Jacobi-era kinds.
 * rank: the columns of L, 1 ... CGX_MAX_PRECOND_RANK (default 32); rank > n is CGX_ERR_BAD_ARG at begin.  shift: delta; 0 (the
 * default) = automatic, the mean of the diagonal of A - L L^T that remains after `rank` steps, summed in a fixed order; a
 * positive finite value is used as given; anything else is CGX_ERR_BAD_ARG.  *delta_used = the shift of the factor in use, 0
 * until a begin has made one for the current matrix, rank and shift.  Both settings belong to the context, survive new matrices,
 * start no GPU work, take effect at the next begin (between begin and end: CGX_ERR_BAD_ARG) and are used only while the kind is
 * CGX_PRECOND_PIVCHOL.  That begin makes the factor on the device once per matrix, rank and shift: at step t the pivot is the
 * not yet chosen row with the largest remaining diagonal (ties: the smallest index), so the pivot sequence is deterministic.  A
 * diagonal entry or a pivot that is not finite and > 0 (the matrix is not positive definite), or a resulting shift that is not
 * finite and > 0, gives CGX_ERR_BAD_ARG (step and row in cgx_last_error) and leaves the context usable.  L takes 8 * rank * lda
 * bytes of device memory; a failed allocation is CGX_ERR_OOM (the size in cgx_last_error). */
enum { CGX_PRECOND_PIVCHOL = 2 };
#define CGX_MAX_PRECOND_RANK 256
cgx_status  cgx_set_preconditioner_rank(cgx_ctx *ctx, int rank);
cgx_status  cgx_get_preconditioner_rank(const cgx_ctx *ctx, int *rank);
cgx_status  cgx_set_preconditioner_shift(cgx_ctx *ctx, double delta);
cgx_status  cgx_get_preconditioner_shift(const cgx_ctx *ctx, double *delta_set, double *delta_used);
/* Storage of local shard `local_shard`: *format = cgx_matrix_format; banded: *ndiag and offsets[0..*ndiag)
 * (column minus row, ascending; room for CGX_MAX_DIAGONALS ints or NULL); *matrix_bytes = device bytes of the block. */
cgx_status  cgx_get_matrix_format(const cgx_ctx *ctx, int local_shard, int *format, int *ndiag, int *offsets,
                                  double *matrix_bytes);
/* Entries stored for local shard `local_shard`: rows * n (dense), ndiag * rows (banded), the shard's nnz (CSR).  CSR's
 * cgx_get_matrix_format gives ndiag = 0 and matrix_bytes = 12 * nnz + 8 * (rows + 1) (values, columns, row pointers). */
cgx_status  cgx_get_matrix_nnz(const cgx_ctx *ctx, int local_shard, long long *nnz);

/* ---- CGSolver::solve, cg.cc:38-156 ------------------------------------------------------- */
/* x: n doubles, in = initial guess (cg_main.cc:49-50 passes zeros), out = solution (every rank
 * gets the full x; the reference fills rank 0 only, cg.cc:140-142).  res may be NULL. */
cgx_status  cgx_solve(cgx_ctx *ctx, double *x, cgx_result *res);

/* The same path cut at its seams, for bench.py's warmup / timed-steps contract:
 *   begin  = cg.cc:49-92 (setup, initial residual GEMV, p0 gather, rsold)
 *   steps  = `nsteps` bodies of the loop cg.cc:96-137 (stops early on convergence); synchronises
 *   end    = cg.cc:140-154 (gather x, DEBUG verification) and fills res. */
cgx_status  cgx_solve_begin(cgx_ctx *ctx, const double *x0);
cgx_status  cgx_solve_steps(cgx_ctx *ctx, int nsteps, int *done_out);
cgx_status  cgx_solve_end(cgx_ctx *ctx, double *x, cgx_result *res);
/* The individual K1 durations (ms, HIP events on the library's stream) of the most recent cgx_solve_steps call, in
 * launch order: at most `cap` are written, *count receives how many exist.  bench.py reports their median. */
cgx_status  cgx_get_gemv_samples(cgx_ctx *ctx, double *ms_out, int cap, int *count);

/* The same for the update kernel (cfg.profile_update): K3 `k_update_xr`, or, under CGX_COMM_P2P with the exchange folded in,
 * `k_update_xr_p2p`, whose duration includes the bounded wait for every peer's chunks (cg.cc:106,135-136). */
cgx_status  cgx_get_update_samples(cgx_ctx *ctx, double *ms_out, int cap, int *count);

/* ---- several right-hand sides against one matrix (one pass over A per iteration serves all of them) ---- */
/* nrhs independent copies of cgx_solve's recurrence (cg.cc:96-137) on the current matrix, one per right-hand side: each column
 * has its own rsold, alpha (with the safeguard of cg.cc:107), beta and break.  A column that breaks keeps its x from then on;
 * the others go on; the loop ends when every column has broken or after max_iter iterations (cgx_set_tolerance /
 * cgx_set_max_iter).  Every iteration reads A ONCE for all columns (csrc/cgx_multi.hip; gemv_variant does not apply).
 * B, X: host arrays, one vector per ROW: B[j*ldb + i], i < n.  X holds the initial guesses on entry and the solutions on return.
 * res: nrhs results (may be NULL), res[j] as cgx_solve's, rel_residual = ||A x_j - b_j|| / ||b_j||; seconds_* are the same in all
 * of them, gemv_ms_* (profile_gemv > 0) and cgx_get_gemv_samples describe the multi-vector K1 launches, gemv_bytes =
 * 8 (n n + 2 nrhs n).  Column j's result depends on (A, b_j, x0_j, nrhs) only: permuting the columns permutes the results bit
 * for bit.  One GPU (CGX_COMM_SELF) and dense storage only, else CGX_ERR_UNSUPPORTED; nrhs outside 1 .. CGX_MAX_RHS, a null
 * pointer, ldb < n, ldx < n or no problem set: CGX_ERR_BAD_ARG.  The single path's plan and state are left as they were. */
#define CGX_MAX_RHS 16
cgx_status  cgx_solve_multi(cgx_ctx *ctx, int nrhs, const double *B, long ldb, double *X, long ldx, cgx_result *res);
/* cgx_solve_multi with the context's preconditioner: arguments, layout, checks and their order are those
 * of cgx_solve_multi.  CGX_PRECOND_NONE: exactly what cgx_solve_multi runs, bit for bit.  CGX_PRECOND_JACOBI with block 1 and
 * CGX_PRECOND_PIVCHOL: every column runs the preconditioned recurrence of cgx_solve (z = M^-1 r, p0 = z0, alpha = r.z / p.Ap with
 * the safeguard, beta = r.z(new) / r.z(old), p = z + beta p) with its own scalars and its own break on sqrt(r.r) < tol;
 * residual_prev / residual_last are sqrt(r.r).  The inverse diagonal / the factor is the single path's, made once per matrix
 * (rank, shift) by whichever call comes first, and whatever a single solve refuses for the kind is refused here with the same
 * status and message (gemv_variant 40000 / 50000, a K1 shape with split columns, rank > n, a matrix that is not positive
 * definite, more than 262144 rows for CGX_PRECOND_PIVCHOL).  Block Jacobi (block > 1): CGX_ERR_UNSUPPORTED.  Column j's result
 * depends on (A, b_j, x0_j, nrhs, the preconditioner's settings) only.
 * cgx_solve_multi itself keeps refusing a preconditioner (CGX_ERR_UNSUPPORTED): callers rely on that refusal to learn that
 * their setting would be ignored, so the preconditioned form is an entry point of its own. */
cgx_status  cgx_solve_multi_pc(cgx_ctx *ctx, int nrhs, const double *B, long ldb, double *X, long ldx, cgx_result *res);
/* The multi-vector K1 alone (plain form): Y_j = A P_j and pAp[j] = P_j . Y_j from the kernel's per-workgroup partials, added
 * in ascending order.  P, Y host arrays, one vector per row (P[j*ldp + i]); pAp: nrhs doubles.  Same scope as cgx_solve_multi. */
cgx_status  cgx_probe_gemv_multi(cgx_ctx *ctx, int nrhs, const double *P, long ldp, double *Y, long ldy, double *pAp);

/* ---- one right-hand side against a family of shifted matrices (one pass over A per iteration serves all shifts) ---- */
/* Multi-shift CG: (A + sigma[j] I) x_j = b for nshift shifts sigma[j] >= 0, from ONE Krylov sequence.  The
 * seed is cgx_solve's recurrence on A itself from x0 = 0 on the per-launch path (K1 + K3 per iteration, any per-launch plan, also
 * where the context's plan is a persistent kernel: that plan is left as it is and the next cgx_solve uses it again); the residual
 * of shift j stays zeta_j r, so every shift costs a scalar recurrence and two vector updates per iteration (csrc/cgx_shift.hip).
 * Inputs: the current matrix and source term, cgx_set_tolerance / cgx_set_max_iter.  The initial guess is zero for every shift
 * (the shifted residuals are collinear only from one common r0 = b): X is output only, one solution per ROW, X[j*ldx + i].
 * Shift j is frozen in iteration k -- converged = 1, iterations = k, nothing writes its x afterwards -- when |zeta_j| sqrt(r.r)
 * < tol, or when |zeta_j| < 2^-500 or is not finite (converged beyond what a double holds).  The loop ends, decided on the device
 * and found by the check_every poll, when the seed breaks in iteration k (every shift still running is then converged at k), when
 * every shift is frozen (the seed need not have converged), or after max_iter iterations (the shifts still running: converged =
 * 0, iterations = max_iter).  res: nshift results (may be NULL): residual_last / residual_prev = |zeta| sqrt(r.r) of the last /
 * previous iteration, x_norm = ||x_j||, rel_residual = the true ||(A + sigma_j I) x_j - b|| / ||b|| from a final mat-vec,
 * seconds_* and gemv_* as cgx_solve_multi fills them, gemv_bytes that of the single K1.  The result of shift j depends on
 * (A, b, sigma_j, tol, max_iter) only: not on the other shifts, their number or order, or check_every; shifts may repeat.
 * sigma = 0 gives the bits of cgx_solve from a zero guess on the per-launch path.
 * One GPU (CGX_COMM_SELF), dense or CSR storage.  CGX_ERR_UNSUPPORTED: more than one rank or CGX_COMM_LOOPBACK, banded storage,
 * a preconditioner set (it breaks the collinearity), gemv_variant 40000 / 50000.  CGX_ERR_BAD_ARG: a null pointer, nshift outside
 * 1 .. CGX_MAX_SHIFTS, ldx < n, a shift that is negative or not finite (its index in cgx_last_error), no matrix or no source
 * term, an open cgx_solve_begin / cgx_solve_end pair.  A failed call leaves the context usable. */
#define CGX_MAX_SHIFTS 16
cgx_status  cgx_solve_shifted(cgx_ctx *ctx, int nshift, const double *sigma, double *X, long ldx, cgx_result *res);

/* ---- symmetric indefinite and negatively shifted systems: MINRES (one pass over A per iteration serves all shifts) ---- */
/* MINRES (Paige and Saunders 1975): (A + sigma[j] I) x_j = b for nshift finite shifts sigma[j] of any sign
 * and size.  A is the current matrix, taken as symmetric and not checked; it need not be definite, and neither need A + sigma I.
 * b is the current source term.  The Lanczos recurrence from r0 = b does not depend on the shift, so one plain K1 launch per
 * iteration (any per-launch plan: general dense, the symmetric upper-triangle kernel, CSR; also where the context's plan is a
 * persistent kernel: that plan is left as it is and the next cgx_solve uses it again) serves every shift, and a shift costs three
 * Givens rotations on scalars and two vector updates per iteration (csrc/cgx_minres.hip).  The initial guess is zero for every
 * shift (one Krylov space from r0 = b serves all shifts): X is output only, one solution per ROW, X[j*ldx + i] -- the sign
 * convention and the argument layout of cgx_solve_shifted, so a caller can switch between the two.
 * Iteration k (0-based) applies column k of the Lanczos matrix; phibar_(k+1), the recurrence's residual norm behind it, falls
 * monotonically and is ||(A + sigma_j I) x_j - b|| in exact arithmetic.  Shift j is frozen in iteration k -- converged = 1,
 * iterations = k, residual_last = |phibar_(k+1)|, residual_prev = |phibar_k|, nothing writes its x afterwards -- when
 * |phibar_(k+1)| < tol (cgx_set_tolerance, absolute, as everywhere).  A Lanczos breakdown in step t (beta_(t+1) <= 2^-36 max
 * |alpha|, cgx_lanczos's rule: the Krylov space is invariant) ends the recurrence: a running shift whose diagonal entry in front
 * of the last rotation is <= 2^-36 (max |alpha| + |sigma_j|) is singular on that space, keeps the x it had and reports converged
 * = 0, iterations = t; every other running shift takes the column and ends with converged = 1, iterations = t, residual_last =
 * 0.  A shift whose rotation or step length is not finite is frozen unconverged without an update of x.  The loop ends, decided
 * on the device and found by the check_every poll, when every shift is frozen, at a breakdown, or after max_iter iterations (the
 * shifts still running: converged = 0, iterations = max_iter, both residuals those of the last two columns).
 * res: nshift results (may be NULL): x_norm = ||x_j||, rel_residual = the true ||(A + sigma_j I) x_j - b|| / ||b|| from a final
 * product as cgx_solve_shifted makes it, seconds_solve and seconds_loop, gemv_bytes that of the single K1; gemv_ms_* and the
 * launch counts stay 0, because plain K1 launches are not event-timed.  The result of shift j depends on (A, b, sigma_j, tol,
 * max_iter, the K1 plan) only: not on the other shifts, their number or order, the kernel width, or check_every; shifts may repeat.
 * One GPU (CGX_COMM_SELF), dense or CSR storage.  CGX_ERR_UNSUPPORTED: more than one rank or CGX_COMM_LOOPBACK, banded storage,
 * a preconditioner set (it would be ignored), gemv_variant 40000 / 50000.  CGX_ERR_BAD_ARG: a null pointer, nshift outside
 * 1 .. CGX_MAX_MINRES_SHIFTS, ldx < n, a shift that is not finite (its index in cgx_last_error), no matrix or no source term, an
 * open cgx_solve_begin / cgx_solve_end pair.  A failed call leaves the context usable and X as it was; a later cgx_solve,
 * cgx_solve_multi or cgx_solve_shifted gives the bits it gave before. */
#define CGX_MAX_MINRES_SHIFTS 16
cgx_status  cgx_solve_minres(cgx_ctx *ctx, int nshift, const double *sigma, double *X, long ldx, cgx_result *res);

/* ---- Lanczos quadrature: log det A, tr(A^-1) and spectrum estimates of the current matrix ---- */
/* The symmetric Lanczos three-term recurrence from nvec start vectors at once, one pass over A per step for all of them
 * (csrc/cgx_lanczos.hip; the mat-vec is cgx_solve_multi's plain multi-vector K1).  Per start vector j:
 *   v_0 = V0_j / ||V0_j||, v_-1 = 0;  step t: y = A v_t, alpha_t = v_t . y, w = y - alpha_t v_t - beta_(t-1) v_(t-1), beta_t = ||w||;
 *   beta_t <= 2^-36 max_(s<=t) |alpha_s|: the column has reached an invariant subspace and is frozen with m_j = t + 1 steps (the
 *   others go on); else v_(t+1) = w / beta_t.
 * There is NO reorthogonalisation: the coefficients are those of the plain recurrence in floating point, which is what Gauss
 * quadrature needs (the Ritz values may repeat once they have converged; the rule stays accurate).
 * V0: host array, one start vector per ROW, V0[j*ldv + i], i < n.  alpha, beta: nvec rows of `steps` doubles (alpha[j*steps + t]);
 * beta[.. + t] = beta_t, the last one included; entries at t >= steps_done[j] are 0; steps_done[j] = m_j.  Column j's result depends
 * on (A, V0_j, steps, the kernel width of nvec: 1, 2, 4, 8 or 16) only: permuting the columns permutes the results bit for bit.
 * One GPU (CGX_COMM_SELF) and dense storage only, else CGX_ERR_UNSUPPORTED; a preconditioner that is set is CGX_ERR_UNSUPPORTED too
 * (the call would ignore it).  CGX_ERR_BAD_ARG: a null pointer, no matrix, nvec outside 1 .. CGX_MAX_RHS, steps < 1, steps > n or
 * steps > CGX_MAX_LANCZOS_STEPS, ldv < n, a start vector of norm 0 or not finite (its column in cgx_last_error).  A failed call
 * leaves the context usable; the single path's plan and state are left as they were. */
#define CGX_MAX_LANCZOS_STEPS 1024
#define CGX_MAX_PROBES 256
enum { CGX_SLQ_LOG = 0, CGX_SLQ_INV = 1 };
cgx_status  cgx_lanczos(cgx_ctx *ctx, int nvec, int steps, const double *V0, long ldv, double *alpha, double *beta, int *steps_done);

/* Stochastic Lanczos quadrature: tr f(A) ~ (1/nprobe) sum_j ||z_j||^2 sum_i tau_i^2 f(theta_i) with (theta, tau) the Ritz values
 * and first eigenvector components of probe j's Jacobi matrix T_j (cgx_tridiag_quadrature), f = log (CGX_SLQ_LOG: log det A) or
 * 1/x (CGX_SLQ_INV: tr A^-1).  Z = NULL: Rademacher probes made by the library, element i of probe j = -1 if the top bit of
 * hash_mix64(hash_mix64(seed) ^ (j << 32 | i)) is set, else +1 (hash_mix64: the splitmix64 finaliser, z += 0x9E3779B97F4A7C15;
 * z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^ z >> 31); else nprobe caller's vectors, one per
 * row (Z[j*ldz + i]; seed is not read).  The probes run through cgx_lanczos's recurrence in batches of 8 (the last batch may be
 * smaller): the value of probe j depends on (A, z_j, steps, the size of its batch) only, so permuting the probes within a batch
 * permutes per_probe bit for bit.  *estimate = the mean over the probes, *std_error = their sample standard deviation /
 * sqrt(nprobe) (0 for one probe); per_probe (nprobe doubles) and ritz (2 doubles: the smallest / largest Ritz value over all
 * probes) may be NULL.  Scope and refusals as cgx_lanczos (ldz is read only with Z); also CGX_ERR_BAD_ARG: nprobe outside
 * 1 .. CGX_MAX_PROBES, an unknown fn, and under either fn a Ritz value <= 0: "matrix is not positive definite", the value in
 * cgx_last_error. */
cgx_status  cgx_trace_slq(cgx_ctx *ctx, int fn, int nprobe, int steps, unsigned long long seed, const double *Z, long ldz,
                          double *estimate, double *std_error, double *per_probe, double *ritz);

/* ---- preconditioned Lanczos quadrature ---- */
/* cgx_lanczos with the context's preconditioner M (M = diag A for CGX_PRECOND_JACOBI with block 1, M = L L^T + delta I for
 * CGX_PRECOND_PIVCHOL), csrc/cgx_lanczos_pc.hip.  Per start vector j:
 *   w_0 = V0_j, u_0 = M^-1 w_0, eta0^2 = w_0 . u_0, v_-1 = 0, beta_-1 := eta0;
 *   step t: v_t = w_t / beta_(t-1), q_t = u_t / beta_(t-1), y = A q_t, alpha_t = q_t . y, w_(t+1) = y - alpha_t v_t - beta_(t-1) v_(t-1),
 *   u_(t+1) = M^-1 w_(t+1), beta_t = sqrt(w_(t+1) . u_(t+1));  beta_t^2 <= 0 or beta_t <= 2^-36 max_(s<=t) |alpha_s|: frozen with
 *   m_j = t + 1.
 * (alpha, beta) are the Jacobi matrix of M^-1/2 A M^-1/2 from the start vector M^-1/2 V0_j, so that V0_j^T M^-1/2 f(M^-1/2 A M^-1/2)
 * M^-1/2 V0_j ~ eta2[j] sum_i tau_i^2 f(theta_i) (cgx_tridiag_quadrature).  No reorthogonalisation.  Arguments, layout and argument
 * errors as cgx_lanczos; eta2: nvec doubles, eta0^2 as the device summed it; a start vector whose eta0^2 is 0, negative or not
 * finite is CGX_ERR_BAD_ARG with its column in cgx_last_error.  Column j's result depends on (A, V0_j, steps, the kernel width of
 * nvec, the preconditioner's settings) only.  CGX_PRECOND_NONE: cgx_lanczos itself, bit for bit, eta2[j] = ||V0_j||^2.
 * Scope and refusals are cgx_solve_multi_pc's, with its statuses, messages and order: one GPU (CGX_COMM_SELF) and dense storage,
 * else CGX_ERR_UNSUPPORTED; block Jacobi, gemv_variant 40000 / 50000 and a K1 shape with split columns: CGX_ERR_UNSUPPORTED; rank >
 * n, a matrix that is not positive definite: CGX_ERR_BAD_ARG.  The inverse diagonal / the factor is the single path's, made once
 * per matrix (rank, shift) by whichever call comes first.  A failed call leaves the context usable; the single path's plan and
 * state are left as they were.  cgx_lanczos and cgx_trace_slq keep refusing a preconditioner. */
cgx_status  cgx_lanczos_pc(cgx_ctx *ctx, int nvec, int steps, const double *V0, long ldv, double *alpha, double *beta, int *steps_done,
                           double *eta2);
/* log det M of the preconditioner that is set (made here if no call has made it yet): CGX_PRECOND_JACOBI the sum of log A_ii in
 * ascending order; CGX_PRECOND_PIVCHOL (n - rank) log delta + log det(delta I + L^T L), the second term from a host Cholesky
 * factorisation of the device's (delta I + L^T L)^-1; CGX_PRECOND_NONE 0.  Scope and refusals as cgx_lanczos_pc. */
cgx_status  cgx_precond_logdet(cgx_ctx *ctx, double *logdet);
/* The nprobe probes that cgx_trace_slq_pc makes itself (Z = NULL) for fn, seed and the preconditioner that is set, one per row
 * (Z[j*ldz + i]).  With s_(j,i) cgx_trace_slq's Rademacher sign of element i of probe j: CGX_SLQ_INV, or CGX_PRECOND_NONE: z = s_j
 * (covariance I).  CGX_SLQ_LOG: covariance M exactly -- Jacobi z_i = s_(j,i) sqrt(A_ii); pivoted Cholesky z = L g + sqrt(delta) s_j
 * with g_c = s_(j, n + c), per row one fma chain over c = 0 .. rank-1 from +0.0, then fma(sqrt(delta), s_(j,i), chain). */
cgx_status  cgx_slq_probes(cgx_ctx *ctx, int fn, int nprobe, unsigned long long seed, double *Z, long ldz);
/* cgx_trace_slq through cgx_lanczos_pc, in batches of 8 probes.
 * CGX_SLQ_LOG: log det A = log det M + tr log(M^-1/2 A M^-1/2); the probes must have covariance M: the library's (Z = NULL, see
 * cgx_slq_probes) or the caller's -- THE CALLER ANSWERS FOR THE COVARIANCE OF ITS OWN PROBES, nothing checks it, and with another
 * covariance the estimate is that of another quantity.  per_probe[j] = eta0^2 sum_i tau_i^2 log theta_i, *estimate = log det M +
 * their mean, *std_error that of the per-probe values, *logdet_precond (may be NULL) = log det M (cgx_precond_logdet).
 * CGX_SLQ_INV: the probes have covariance I (Z = NULL: cgx_trace_slq's Rademacher vectors, bit for bit); per_probe[j] = eta0^2
 * sum_i tau_i^2 / theta_i = z_j^T A^-1 z_j, *estimate their mean, *logdet_precond = 0.  The preconditioner cuts the steps needed.
 * ritz: the extreme Ritz values of M^-1/2 A M^-1/2.  CGX_PRECOND_NONE: cgx_trace_slq itself, bit for bit, *logdet_precond = 0.
 * Scope and refusals as cgx_lanczos_pc, argument errors as cgx_trace_slq; a Ritz value <= 0: CGX_ERR_BAD_ARG "matrix is not
 * positive definite", the value in cgx_last_error. */
cgx_status  cgx_trace_slq_pc(cgx_ctx *ctx, int fn, int nprobe, int steps, unsigned long long seed, const double *Z, long ldz,
                             double *estimate, double *std_error, double *per_probe, double *ritz, double *logdet_precond);

/* HOST ONLY, no context: nodes and weights of the m-point Gauss rule of the Jacobi matrix with diagonal alpha[0..m) and
 * off-diagonal beta[0..m-1) (beta may be NULL for m = 1): theta ascending, weight_i = (first component of eigenvector i)^2.
 * Implicit symmetric QL on the first row of the eigenvector matrix alone, O(m^2), no LAPACK.  CGX_ERR_BAD_ARG: m < 1, a null
 * pointer, an entry that is not finite.  CGX_ERR_UNSUPPORTED: a value did not converge within 60 sweeps (not seen so far). */
cgx_status  cgx_tridiag_quadrature(int m, const double *alpha, const double *beta, double *theta, double *weight);

/* ---- a matrix function applied to vectors: A^(1/2) b, A^(-1/2) b, A^-1 b, log(A) b, exp(-tau A) b ---- */
/* HOST ONLY, no context: coef[t] = (f(T) e_1)_t, t < m, for the Jacobi matrix T of cgx_tridiag_quadrature's arguments (beta may be
 * NULL for m = 1) and f(theta) = sqrt(theta) (CGX_FN_SQRT), 1 / sqrt(theta) (CGX_FN_INVSQRT), 1 / theta (CGX_FN_INV), log(theta)
 * (CGX_FN_LOG) or exp(-param theta) (CGX_FN_EXP; param is read for this function only and must be finite and >= 0).  The implicit
 * QL sweep of cgx_tridiag_quadrature with every plane rotation of the first row recorded; f(T) e_1 is those rotations applied in
 * reverse to f(d_k) z_k: O(m^2) time, about 1.1 m^2 recorded rotations of transient memory, no LAPACK.  theta_minmax (may be NULL)
 * receives the smallest and largest eigenvalue of T, also when the call fails for the domain.  CGX_ERR_BAD_ARG: m < 1, a null
 * pointer, an entry that is not finite, an unknown fn, a bad param, an eigenvalue outside the function's domain (theta < 0 for
 * CGX_FN_SQRT; theta <= 0 for CGX_FN_INVSQRT, CGX_FN_INV, CGX_FN_LOG).  CGX_ERR_UNSUPPORTED: no convergence within 60 sweeps. */
enum { CGX_FN_SQRT = 0, CGX_FN_INVSQRT = 1, CGX_FN_INV = 2, CGX_FN_LOG = 3, CGX_FN_EXP = 4 };
cgx_status  cgx_tridiag_function(int m, const double *alpha, const double *beta, int fn, double param, double *coef,
                                 double *theta_minmax);
/* X_j ~ f(A) B_j for nvec <= CGX_MAX_RHS vectors, one per ROW (B[j*ldb + i], X[j*ldx + i]), by `steps` steps of Lanczos: with V_m
 * the Lanczos vectors of B_j and T_m their Jacobi matrix, x = ||b|| V_m f(T_m) e_1.  The recurrence is cgx_lanczos's, bit for bit
 * (the same kernels, kernel width and freezing rule, m_j = the steps column j made), with the normalised v_t of every step kept on
 * the device: 8 steps nvec lda bytes (4.3 GB at n = 32768, 16 vectors, 1024 steps), a block of its own that is made on first use,
 * made again when a call needs more and freed with the problem; a failed allocation is CGX_ERR_OOM with the size in
 * cgx_last_error and leaves the context usable.  No reorthogonalisation.  c_j = sqrt(z2_j) cgx_tridiag_function(m_j, alpha_j,
 * beta_j, fn, param), one multiplication per entry, z2_j = ||B_j||^2 as the device summed it; X_j[i] = sum over t < m_j of
 * c_j[t] v_(j,t)[i], ONE fma chain per element in ascending t from +0.0 (csrc/cgx_funm.hip).  From 64 steps on the columns'
 * coefficients are made on one host thread per column (up to nvec x 30 MB of transient host memory at 1024 steps).  Column j's
 * result depends on (A, B_j, fn, param, steps, the kernel width of nvec: 1, 2, 4, 8 or 16) only: permuting the columns permutes
 * X bit for bit.
 * steps_done (nvec ints: m_j), change (nvec doubles) and coef (nvec rows of `steps` doubles: c_j, zero at t >= m_j) may each be
 * NULL; X is written only when the call succeeds.  change[j] is a convergence INDICATOR, not a bound: with m = m_j and lag = m -
 * max(1, m / 8) (integer division), || c(m) - pad(c(lag)) || / || c(m) || with c(lag) made from the leading lag x lag block of T, sums
 * in ascending t; 1 when lag = 0, 0 when || c(m) || = 0.  In exact arithmetic it is || x_m - x_lag || / || x_m ||.
 * One GPU (CGX_COMM_SELF) and dense storage only, else CGX_ERR_UNSUPPORTED; a preconditioner that is set is CGX_ERR_UNSUPPORTED too
 * (f(M^-1/2 A M^-1/2) is another quantity).  CGX_ERR_BAD_ARG: no matrix, steps < 1, steps > n or steps > CGX_MAX_LANCZOS_STEPS,
 * nvec outside 1 .. CGX_MAX_RHS, a null B or X, ldb < n or ldx < n, an unknown fn or a bad param (all before any GPU work), a start
 * vector of norm 0 or not finite (its column in cgx_last_error), a Ritz value outside the function's domain: "matrix is not
 * positive definite", the value and the column in cgx_last_error.  A failed call leaves the context usable; the single path's
 * plan and state are left as they were. */
cgx_status  cgx_apply_function(cgx_ctx *ctx, int fn, double param, int nvec, int steps, const double *B, long ldb, double *X, long ldx,
                               int *steps_done, double *change, double *coef);
/* TEST PROBE: the combine kernel of cgx_apply_function by itself.  Q[((size_t)t*nvec + j)*ldq + i] is the caller's basis (steps
 * slots of nvec vectors), C nvec rows of `steps` coefficients, m nvec step counts in 0 .. steps: X_j[i] = sum over t < m[j] of
 * C[j*steps + t] Q[..], as above; slots at t >= m[j] are not read.  Same scope as cgx_apply_function (a problem must be set: it
 * gives n and the row pitch). */
cgx_status  cgx_probe_funm_combine(cgx_ctx *ctx, int nvec, int steps, const int *m, const double *Q, long ldq, const double *C,
                                   double *X, long ldx);

/* ---- extreme eigenpairs: Lanczos with full reorthogonalisation ---- */
enum { CGX_EIG_LARGEST = 0, CGX_EIG_SMALLEST = 1 };
#define CGX_MAX_EIGENPAIRS 16
/* HOST ONLY, no context: eigenvalues and selected eigenvectors of the Jacobi matrix T of cgx_tridiag_quadrature's arguments (beta may
 * be NULL for m = 1).  theta (m doubles, may be NULL) receives all eigenvalues in ascending order; index[c], c < nsel, is in 0 .. m-1
 * and counts in that order (repeats are allowed); row c of S (nsel rows of m doubles) is the unit eigenvector of index[c], signed so
 * that its first component is >= 0.  The recorded QL sweep of cgx_tridiag_function: eigenvector k is the recorded rotations applied
 * in reverse to e_k, O(m^2) per vector, nothing m x m is held, no LAPACK.  CGX_ERR_BAD_ARG: m < 1, a null alpha, S or index, a null
 * beta with m > 1, an entry that is not finite, nsel < 1, an index out of range.  CGX_ERR_UNSUPPORTED: no convergence within 60
 * sweeps. */
cgx_status  cgx_tridiag_eigenvectors(int m, const double *alpha, const double *beta, int nsel, const int *index,
                                    double *theta, double *S);
/* The nev largest (CGX_EIG_LARGEST) or smallest (CGX_EIG_SMALLEST) eigenvalues of the current matrix and their eigenvectors, from at
 * most `steps` steps of Lanczos on ONE start vector with the basis kept orthogonal (csrc/cgx_eigs.hip).  A is taken as symmetric
 * (not checked) and need not be positive definite.  v0: n doubles, or NULL for probe 0 of cgx_trace_slq's Rademacher hash of `seed`
 * (seed is not read otherwise).  With q_0 = v0 / ||v0||, step t:
 *   y = A q_t (cgx_solve_multi's plain K1 at width 1), alpha_t = q_t . y from its partials in a fixed order;
 *   w = y - alpha_t q_t - beta_(t-1) q_(t-1);  twice: h = Q_t^T w over slots 0 .. t, w = w - Q_t h (classical Gram-Schmidt, twice:
 *   per slot the partials of 256-row tiles added in ascending tile order, per element one fma chain over the slots in ascending
 *   order from +0.0);  beta_t = ||w||;  beta_t <= 2^-36 max_(s<=t) |alpha_s|: the space is invariant, the run is frozen with m = t + 1
 *   (decided on the device: the launches behind it exit at once); else q_(t+1) = w / beta_t.
 * T_m has alpha as first computed and beta behind the reorthogonalisation.  tol = 0: all `steps` steps run.  tol > 0: behind every
 * step with (t + 1) mod 16 = 0, and behind the last one, the host reads alpha and beta, forms the wanted Ritz pairs of T and
 * estimate_j = beta_t |s_(t,j)| (s_j: the unit eigenvector of T, its last component) and stops once every wanted estimate is <=
 * tol max |theta| over all Ritz values of T.
 * values[j], j < nev: descending for CGX_EIG_LARGEST, ascending for CGX_EIG_SMALLEST.  vectors[j*ldv + i] = sum over t < m of
 * s_j[t] q_t[i], one fma chain per element in ascending t from +0.0, the sign that of s_j[0] >= 0; the basis is read once for all
 * nev vectors.  residual[j] = ||A x_j - theta_j x_j|| from one more plain K1 on the nev vectors: a true residual, the basis is not
 * used for it.  estimate[j] as above.  *steps_done = m; *nfound = min(nev, m), and entries at j >= nfound are 0.  vectors, residual,
 * estimate, steps_done and nfound may each be NULL; outputs are written only when the call succeeds.  The result depends on (A, v0
 * or seed, which, nev, steps, tol) only, and a run of more steps has the shorter run's alpha_t, beta_t and q_t as a bitwise prefix.
 * With an exactly multiple eigenvalue a single start vector finds ONE vector of its eigenspace (the Krylov space holds no more):
 * the value comes back once, and the next entry is the next distinct eigenvalue.  No restarts: the basis takes 8 (steps + 1) lda
 * bytes on the device in a block of its own, made on first use, made again when a call needs more, freed with the problem; a
 * failed allocation is CGX_ERR_OOM with the size in cgx_last_error.
 * Scope, checks and their order are cgx_lanczos's: one GPU (CGX_COMM_SELF), dense storage and no preconditioner set, else
 * CGX_ERR_UNSUPPORTED; steps in 1 .. min(n, CGX_MAX_LANCZOS_STEPS), else CGX_ERR_BAD_ARG.  Then CGX_ERR_BAD_ARG before any GPU work:
 * an unknown `which`, nev outside 1 .. CGX_MAX_EIGENPAIRS or > steps, tol negative or not finite, a null values, ldv < n with vectors
 * given; and from the device a start vector of norm 0 or not finite.  A failed call leaves the context usable; the single path's
 * plan and state and the blocks of the other entry points are left as they were. */
cgx_status  cgx_eigenpairs(cgx_ctx *ctx, int which, int nev, int steps, double tol, const double *v0,
                          unsigned long long seed, double *values, double *vectors, long ldv,
                          double *residual, double *estimate, int *steps_done, int *nfound);
/* TEST PROBE: the recurrence of cgx_eigenpairs alone (tol = 0) from v0 (not NULL).  alpha, beta: `steps` doubles, zero at t >=
 * *steps_done = m.  Q[t*ldq + i] receives slots 0 .. m-1 and, when no step froze the run (then m = steps), also slot m, the next
 * vector: Q must hold steps + 1 rows; rows that are not written keep what they held.  Scope and refusals as cgx_eigenpairs. */
cgx_status  cgx_probe_eigs_basis(cgx_ctx *ctx, int steps, const double *v0, double *Q, long ldq,
                                double *alpha, double *beta, int *steps_done);
/* TEST PROBE: ONE projection + subtraction pass of cgx_eigenpairs on the caller's slots Q[s*ldq + i], s < nslots <=
 * CGX_MAX_LANCZOS_STEPS, and w_in (n doubles): h_out[s] = q_s . w_in, w_out = w_in - sum_s h_out[s] q_s, in the kernels' orders.  On
 * the device the slots, the slot behind them and the vector are filled with NaN over their whole row pitch before the upload.  A
 * problem must be set (it gives n and the row pitch); one GPU and dense storage. */
cgx_status  cgx_probe_eigs_orthogonalise(cgx_ctx *ctx, int nslots, const double *Q, long ldq,
                                        const double *w_in, double *w_out, double *h_out);

/* ---- kernel probes (parity tests of the individual hot ops through the C ABI) ------------- */
/* Ap = A_shard * p  (K1; cblas_dgemv at cg.cc:101-102) for every local shard; y receives the n
 * results in global row order (LOOPBACK/SELF) or this rank's rows at their global offset (RCCL);
 * *pAp receives sum_i p_i * Ap_i over the local rows (the fused cblas_ddot of cg.cc:105). */
cgx_status  cgx_probe_gemv(cgx_ctx *ctx, const double *p, double *y, double *pAp);
/* Mean duration (ms, HIP events) of `reps` back-to-back launches of the plain K1 on the current matrix. */
cgx_status  cgx_probe_time_gemv(cgx_ctx *ctx, int reps, double *ms_per_launch);
/* One pass of K3 (cg.cc:107-116) and of the p update fused into the next K1 (cg.cc:124-129) on caller
 * data of length n, single shard: x += alpha p; r -= alpha Ap; *rr = r.r; p = r + beta p. */
cgx_status  cgx_probe_vector_ops(cgx_ctx *ctx, int n, double alpha, double beta, double *x, double *r,
                                 double *p, const double *Ap, double *rr);
/* Error-path testing: after `calls` further HIP runtime calls of this context the next one is not made and reports a
 * failure instead (-1 = off).  TEST-ONLY: tools/leak_check.py and tests/ use it to walk every early return of a probe,
 * the self-test and the solve; nothing else (no environment variable) arms it. */
cgx_status  cgx_probe_set_fault_after(cgx_ctx *ctx, int calls);
/* The Matrix-Market parser of cgx_read_matrix by itself, HOST ONLY (no context, no device): header checks as
 * matrix_coo.cc:19-40, then the nz entries "%d %d %lg" (matrix_coo.cc:44-55) parsed from the mapped file on `threads` host
 * threads (0 = the library's default; negative = exactly that many, however small the file) into 0-based I, J and a in
 * file order; at most `cap` entries are written (call with cap = 0 for the sizes).  err (may be NULL) receives the message. */
cgx_status  cgx_probe_parse_matrix_market(const char *path, int threads, int *m, int *n, int *nz, int *symmetric, int *I, int *J,
                                          double *a, long cap, char *err, int err_cap);
/* TEST ONLY: moves the mailbox of a ONE-rank CGX_COMM_P2P context (no problem set yet) into pinned, coherent host memory, so
 * that every store, poll and load of the exchange crosses PCIe: the system-scope path outside this GPU's HBM and L2. */
cgx_status  cgx_probe_p2p_mailbox_to_host(cgx_ctx *ctx);
/* TEST ONLY: the mailboxes of a multi-rank CGX_COMM_P2P job in POSIX shared HOST memory (segments <prefix>_<rank>), so that
 * the stores, polls and loads of EVERY rank cross PCIe between separate processes -- the closest a one-GPU box offers to
 * peers whose memory is remote.  Replaces cgx_p2p_export / cgx_p2p_import: stage 0 creates this rank's segment and makes it
 * the mailbox; after a launcher barrier stage 1 maps every peer's.  Before any problem is set. */
cgx_status  cgx_probe_p2p_host_mailboxes(cgx_ctx *ctx, const char *prefix, int stage);
/* Test hook for the co-residency guard of CGX_COMM_P2P's fused update kernel (its workgroups wait for each other inside the
 * kernel, so its grid must not exceed what the device keeps resident: occupancy x CUs, queried from the runtime when a
 * problem is set): workgroups > 0 replaces the queried bound for the problems set afterwards, 0 restores it.  The same bound
 * guards the LDS-resident solver (its workgroups wait for each other as well): with a bound below its grid the default falls
 * back to the per-launch path and gemv_variant 40000 is refused. */
cgx_status  cgx_probe_set_resident_limit(cgx_ctx *ctx, int workgroups);
/* TEST ONLY, host arithmetic (no device, no context): the shape the library would give a persistent kernel for a dense n x n
 * problem on a GPU of `cus` compute units with `lds_per_cu` bytes of LDS a workgroup may use -- streaming = 0: the resident
 * kernel (n <= 4096), 1: the streaming kernel (1024 <= n <= 16384).  out = {fits (0 / 1), R rows per workgroup, S column steps,
 * grid, exchange slots per parity, LDS bytes per workgroup, rows in LDS, rows in registers, rows per batch of the ring
 * (streaming), streamed rows read with the default cache policy (streaming), hybrid (resident: 1 = rows in LDS + registers + a
 * streamed rest), threads per workgroup}.  tests/test_persistent_plans.py holds the invariants for every n. */
#define CGX_PERSISTENT_PLAN_INTS 12
cgx_status  cgx_probe_persistent_plan(int n, int cus, long lds_per_cu, int streaming, long out[CGX_PERSISTENT_PLAN_INTS]);
/* TEST ONLY: the epoch counter of mailbox channel `chan` (0 = plain segment all-gathers of a tagged-word context, 1 = the
 * iteration's exchange, 2 = DEBUG scalars).  set: move it FORWARD to `value` (the next exchange is value + 1) so that tests
 * reach the wrap of the tagged form's 32-bit tag and of the epoch's low 32 bits without 4e9 exchanges; every rank makes the
 * same call between two solves.  A smaller value is refused (flag words only grow). */
cgx_status  cgx_probe_set_p2p_epoch(cgx_ctx *ctx, int chan, unsigned long long value);
cgx_status  cgx_probe_get_p2p_epoch(cgx_ctx *ctx, int chan, unsigned long long *value);
/* TEST ONLY, the resident solver (gemv_variant 0 / 40000, n <= 4096 on one GPU).  epoch > 0: move the epoch counter of
 * its tagged-word exchange FORWARD to `epoch` (the next iteration uses epoch + 1), so that tests reach the wrap of the 32-bit
 * tag without 4e9 iterations; a smaller value is refused.  mute_workgroup >= 0: that workgroup of the NEXT launch leaves out the
 * publish of its first iteration, so that every wait for it expires (the bounded-wait path: cgx_solve_steps then returns
 * CGX_ERR_HIP after p2p_timeout_ms); -1 = none.  The mute disarms itself after one launch. */
cgx_status  cgx_probe_resident_test(cgx_ctx *ctx, unsigned long long epoch, int mute_workgroup);
/* Copy the device-resident source term of local shard `local_shard` (n doubles, what cgx_init_source_term /
 * cgx_set_source_term left in HBM) back to the host: the bit-exact check of cg.cc:230-231. */
cgx_status  cgx_probe_get_source_term(cgx_ctx *ctx, int local_shard, double *b_out);
/* TEST ONLY: dense, incompressible data for K1 at the BASELINE sizes.  The reference's generator leaves 5 non-zeros per row
 * (cg.cc:178-186) while its GEMV is a general dense dgemv (cg.cc:101-102): this call overwrites the dense row block of every
 * local shard of the CURRENT problem (set one first: it defines n, the partition and the pitch) on the device with
 * A(i,j) = (double)(mix64(mix64(seed) ^ (i << 32 | j)) >> 11) * 2^-52 - 1 in [-1, 1), mix64 = the splitmix64 finaliser
 * (csrc/cgx_kernels.h hash_entry; the parity tests restate it so that a checker rebuilds any row on the host).
 * symmetric != 0: (i,j) and (j,i) share the value of (min, max).  diag != 0: A(i,i) = diag. */
cgx_status  cgx_probe_fill_matrix_hash(cgx_ctx *ctx, unsigned long long seed, int symmetric, double diag);
/* TEST ONLY: the replicated block inverses of local shard `local_shard` as n rows of `block` doubles: row i, entry t =
 * (D_b^-1)(i, s(i) + t) with s(i) = i - i mod block (0 outside a truncated last block).  Valid after a cgx_solve_begin with a
 * block size > 1; otherwise CGX_ERR_BAD_ARG. */
cgx_status  cgx_probe_get_precond_blocks(cgx_ctx *ctx, int local_shard, double *W_out);
/* TEST ONLY: the factor of CGX_PRECOND_PIVCHOL: pivots[0 .. rank) = the pivot rows in the order chosen, L_out = n rows of rank
 * doubles (row i, entry t = L[i][t]), *delta_used = the shift in use.  cgx_probe_precond_apply: z = P^-1 r for a caller's vector
 * (n doubles each) through the device code the loop runs.  Both are valid after a cgx_solve_begin with the kind set; otherwise
 * CGX_ERR_BAD_ARG. */
cgx_status  cgx_probe_get_precond_lowrank(cgx_ctx *ctx, int *pivots, double *L_out, double *delta_used);
cgx_status  cgx_probe_precond_apply(cgx_ctx *ctx, const double *r, double *z);
/* TEST ONLY: Z_j = M^-1 R_j for nrhs vectors (one per row, as cgx_solve_multi_pc's B and X) through the set-up form of the
 * preconditioned multi-vector update kernels.  Needs CGX_PRECOND_JACOBI (block 1) or CGX_PRECOND_PIVCHOL; makes the inverse
 * diagonal / the factor if the current matrix has none yet. */
cgx_status  cgx_probe_multi_pc_apply(cgx_ctx *ctx, int nrhs, const double *R, long ldr, double *Z, long ldz);
/* Copy this shard's device row block (rows x n, dense, row-major) back to the host (banded storage is expanded). */
cgx_status  cgx_probe_get_matrix_rows(cgx_ctx *ctx, int local_shard, double *A_out, int *row0, int *rows);

#ifdef __cplusplus
}
#endif
#endif /* CGX_H */
