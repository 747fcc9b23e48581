// cgx_precond.cpp -- the set-up of the preconditioners, inside cgx_solve_begin: point Jacobi, block Jacobi
// (section 13) and the pivoted-Cholesky low-rank factor (section 15).  Set-up code only: the loop's kernels take dinv / W / L as
// arguments (enqueue_iteration, cgx_solve.cpp).
#include "cgx_internal.h"

#include <algorithm>
#include <climits>
#include <cstdio>

using namespace cgxi;

namespace {

// The word the check kernels lower to the first row they cannot take: armed above every row index, before them ...
cgx_status arm_jbad(cgx_ctx *ctx)
{
    if (!ctx->d_jbad) HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(&ctx->d_jbad), sizeof(int)));
    HIP_TRY(ctx, hipMemsetAsync(ctx->d_jbad, 0x7f, sizeof(int), ctx->stream));   // 0x7f7f7f7f
    return CGX_OK;
}

// ... and read back behind them: *bad = that row, or -1 where every row passed.
cgx_status read_jbad(cgx_ctx *ctx, int *bad)
{
    *bad = INT_MAX;
    HIP_TRY(ctx, hipMemcpyAsync(bad, ctx->d_jbad, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (*bad < 0 || *bad >= ctx->n) *bad = -1;
    return CGX_OK;
}

// The replicated z of a shard, [z | r.z partials | r.r partials] in rv's geometry: made at the first preconditioned solve of a
// problem, whichever kind asks first.
cgx_status ensure_zbuf(cgx_ctx *ctx, Shard &s)
{
    if (!s.zbuf) {
        const size_t zbytes = (size_t)(s.rv.S + (s.rv.S - s.rv.Sr)) * sizeof(double);
        HIP_TRY(ctx, hipMalloc(&s.zbuf, zbytes));
        HIP_TRY(ctx, hipMemsetAsync(s.zbuf, 0, zbytes, ctx->stream));
    }
    s.zv = s.rv;
    s.zv.base = s.zbuf;
    return CGX_OK;
}

// ---- block-Jacobi set-up -----------------------------------------------------
// Behind prepare_jacobi's refusals and buffers, once per matrix and block size: W (block x lda doubles per shard, replicated like
// dinv).  For t = 0 ... block-1 every shard writes column t of its own block rows into its Ap slice, the segment exchange gathers
// the slices as it gathers the diagonal, and every shard unpacks them into W's row t (one rank: one launch writes all of W).
// Then every shard inverts every block from its gathered copy, on the device, so all ranks take the same decision, after the
// last exchange.
cgx_status prepare_block_jacobi(cgx_ctx *ctx)
{
    const int block = ctx->precond_block;
    if (ctx->cfg.comm_mode == CGX_COMM_P2P && !ctx->cfg.p2p_separate_exchange)
        return fail(ctx, CGX_ERR_UNSUPPORTED,
                    "block Jacobi: the update kernel with the peer exchange inside has no block form (p2p_separate_exchange = 1 has)");
    hipStream_t st = ctx->stream;
    const size_t wbytes = (size_t)block * (size_t)ctx->lda * sizeof(double);
    for (auto &s : ctx->shards) {
        if (s.W && s.w_block != block) {
            ctx->dinv_valid = false;
            HIP_TRY(ctx, hipFree(s.W));
            s.W = nullptr;
            s.w_block = 0;
        }
        if (!s.W) {
            ctx->dinv_valid = false;
            const hipError_t e = fault_due(ctx) ? hipErrorUnknown : hipMalloc(&s.W, wbytes);
            if (e != hipSuccess) {
                s.W = nullptr;
                quiesce(ctx);
                char msg[200];
                snprintf(msg, sizeof msg, "block Jacobi: %zu bytes of block inverses (8 x block %d x pitch %ld) could not be allocated: %s",
                         wbytes, block, ctx->lda, hipGetErrorString(e));
                return fail(ctx, e == hipErrorOutOfMemory ? CGX_ERR_OOM : CGX_ERR_HIP, msg);
            }
            s.w_block = block;
        }
    }
    if (ctx->dinv_valid) return CGX_OK;
    const bool one = ctx->shards.size() == 1 && ctx->nranks == 1;
    auto slice = [&](Shard &s, int t0, int nt, double *dst, long stride) -> cgx_status {
        if (ctx->csr) HIP_TRY(ctx, cgx::launch_csr_bj_col_slice(s.csr, ctx->n, s.rows, s.row0, block, t0, nt, dst, stride, st));
        else HIP_TRY(ctx, cgx::launch_bj_col_slice(s.A, ctx->lda, ctx->n, s.rows, s.row0, block, t0, nt, dst, stride, st));
        return CGX_OK;
    };
    if (one) {
        Shard &s = ctx->shards[0];
        HIP_TRY(ctx, hipMemsetAsync(s.W, 0, wbytes, st));   // the pad rows
        CGX_TRY(slice(s, 0, block, s.W, ctx->lda));
    } else {
        for (int t = 0; t < block; ++t) {
            for (auto &s : ctx->shards) CGX_TRY(slice(s, t, 1, s.Ap(), 0));
            CGX_TRY(gather_segments(ctx, false));
            for (auto &s : ctx->shards) HIP_TRY(ctx, cgx::launch_unpack_segments(s.apv, s.W + (size_t)t * ctx->lda, ctx->lda, st));
        }
    }
    CGX_TRY(arm_jbad(ctx));
    for (auto &s : ctx->shards) HIP_TRY(ctx, cgx::launch_bj_invert(s.W, ctx->lda, ctx->n, block, ctx->d_jbad, st));
    int bad = -1;
    CGX_TRY(read_jbad(ctx, &bad));
    if (bad >= 0) {
        char msg[200];
        snprintf(msg, sizeof msg, "block Jacobi: the %d x %d diagonal block that begins at row %d is not positive definite "
                                  "(a pivot of its factorisation is not finite and > 0)", block, block, bad);
        return fail(ctx, CGX_ERR_BAD_ARG, msg);
    }
    ctx->dinv_valid = true;
    return CGX_OK;
}

}  // namespace

namespace cgxi {

// ---- Jacobi set-up -----------------------------------------------------------
// Collective, inside cgx_solve_begin: the refusals, the buffers, and -- once per matrix -- the diagonal.  Every shard reads the
// diagonal of its own rows into its Ap slice, the transport's segment exchange gathers the slices, and every shard forms the
// replicated dinv from its gathered copy.  The check (finite and > 0) runs on that copy, so all ranks take the same decision,
// and only after the exchange, so no rank is left waiting in it.
cgx_status prepare_jacobi(cgx_ctx *ctx)
{
    if (ctx->banded) return fail(ctx, CGX_ERR_UNSUPPORTED, "Jacobi preconditioner: banded storage is not supported");
    if (ctx->res_forced)
        return fail(ctx, CGX_ERR_UNSUPPORTED, "Jacobi preconditioner: the persistent kernels (gemv_variant 40000 / 50000) have no Jacobi form");
    hipStream_t st = ctx->stream;
    for (auto &s : ctx->shards) {
        if (!s.dinv) HIP_TRY(ctx, hipMalloc(&s.dinv, (size_t)ctx->lda * sizeof(double)));
        CGX_TRY(ensure_zbuf(ctx, s));
    }
    if (ctx->precond_block > 1) return prepare_block_jacobi(ctx);
    if (ctx->dinv_valid) return CGX_OK;
    for (auto &s : ctx->shards) {
        if (ctx->csr)   // the entry with col == row, 0 where the row has none (then refused below like any entry <= 0)
            HIP_TRY(ctx, cgx::launch_csr_diag_slice(s.csr, s.rows, s.row0, s.Ap(), st));
        else
            HIP_TRY(ctx, cgx::launch_diag_slice(s.A, ctx->lda, s.rows, s.row0, s.Ap(), st));
    }
    CGX_TRY(gather_segments(ctx, false));
    CGX_TRY(arm_jbad(ctx));
    for (auto &s : ctx->shards) HIP_TRY(ctx, cgx::launch_jacobi_dinv(s.apv, ctx->n, ctx->lda, s.dinv, ctx->d_jbad, st));
    int bad = -1;
    CGX_TRY(read_jbad(ctx, &bad));
    if (bad >= 0) {
        const Shard &s = ctx->shards[0];
        const int nl = s.apv.n_loc, P = s.apv.nranks;
        const int q = nl > 0 ? std::min(bad / nl, P - 1) : P - 1;
        double v = 0.0;
        HIP_TRY(ctx, hipMemcpy(&v, s.apg + bad + (long)q * s.apv.seg_gap, sizeof(double), hipMemcpyDeviceToHost));
        char msg[160];
        snprintf(msg, sizeof msg, "Jacobi preconditioner: diagonal entry of row %d is %.17g (every entry must be finite and > 0)", bad, v);
        return fail(ctx, CGX_ERR_BAD_ARG, msg);
    }
    ctx->dinv_valid = true;
    return CGX_OK;
}

// ---- pivoted-Cholesky set-up -------------------------------------------------
namespace {

void carve_lr(Carver &c, long lda, int n, cgx::LrWork *w)
{
    w->d = c.take((size_t)lda);
    w->cand_v = c.take(2 * (size_t)cgx::kMaxVectorGrid);
    w->cand_i = reinterpret_cast<int *>(c.take((size_t)cgx::kMaxVectorGrid));   // 2 x kMaxVectorGrid ints
    w->piv = reinterpret_cast<int *>(c.take((size_t)cgx::kLrMaxRank / 2));
    w->C = c.take((size_t)cgx::kLrLd * cgx::kLrLd);
    w->tpart = c.take((size_t)cgx::lr_grid(n) * cgx::kLrLd);
    w->head = c.take_struct<cgx::LrHead>();
}

}  // namespace

cgx::LrWork lr_work(const cgx_ctx *ctx)
{
    cgx::LrWork w{};
    Carver c{ctx->lr_block};
    carve_lr(c, ctx->lda, ctx->n, &w);
    return w;
}

cgx::PcFactor pc_factor(const cgx_ctx *ctx, double *tpart)
{
    cgx::PcFactor f{};
    if (ctx->precond == CGX_PRECOND_JACOBI) {
        f.dinv = ctx->shards[0].dinv;
    } else {
        const cgx::LrWork w = lr_work(ctx);
        f.L = ctx->lr_L;
        f.rank = ctx->lr_L_rank;
        f.Cinv = w.C;
        f.head = w.head;
        f.tpart = tpart;
    }
    return f;
}

// One GPU, inside cgx_solve_begin: the refusals, the buffers, and -- once per matrix, rank and shift -- the factor: rank launches
// of the step kernel, delta, C = delta I + L^T L and its inverse (block Jacobi's sweep on one block), all in stream order; the
// head (failed step / row, delta) and the inversion's word are read back once behind the last of them.
cgx_status prepare_lowrank(cgx_ctx *ctx)
{
    const char *who = "pivoted-Cholesky preconditioner: ";
    if (ctx->cfg.comm_mode != CGX_COMM_SELF || ctx->nranks != 1 || ctx->shards.size() != 1)
        return fail(ctx, CGX_ERR_UNSUPPORTED, std::string(who) + "one rank with comm_mode CGX_COMM_SELF only (the pivot search and the "
                                                                  "loop's kernels have no exchange)");
    if (ctx->banded || ctx->csr) return fail(ctx, CGX_ERR_UNSUPPORTED, std::string(who) + "dense storage only");
    if (ctx->res_forced)
        return fail(ctx, CGX_ERR_UNSUPPORTED, std::string(who) + "the persistent kernels (gemv_variant 40000 / 50000) have no preconditioned form");
    // a K1 shape that leaves Ap as column pieces (gemv_variant 1xxx3 / 4 / 5) needs the prefold kernel in front of the update kernel:
    // the loop's update kernel here reads Ap and K1's own partials as K1 leaves them
    if (ctx->chunked)   // (set for such a shape on one GPU too; the symmetric K1's plan.split counts tile rows, not pieces)
        return fail(ctx, CGX_ERR_UNSUPPORTED, std::string(who) + "a K1 shape with split columns (gemv_variant ending in 3, 4 or 5) is not supported");
    const int n = ctx->n, rank = ctx->precond_rank;
    if ((long)cgx::lr_grid(n) > cgx::kMaxVectorGrid)
        return fail(ctx, CGX_ERR_UNSUPPORTED, std::string(who) + "more than 262144 rows");
    if (rank > n)
        return fail(ctx, CGX_ERR_BAD_ARG, std::string(who) + "rank " + std::to_string(rank) + " exceeds the " + std::to_string(n) + " rows of the matrix");
    Shard &s = ctx->shards[0];
    hipStream_t st = ctx->stream;
    CGX_TRY(ensure_zbuf(ctx, s));
    const size_t lbytes = (size_t)rank * (size_t)ctx->lda * sizeof(double);
    if (ctx->lr_L && ctx->lr_L_rank != rank) {
        ctx->lr_valid = false;
        HIP_TRY(ctx, hipFree(ctx->lr_L));
        ctx->lr_L = nullptr;
        ctx->lr_L_rank = 0;
    }
    if (!ctx->lr_L) {
        ctx->lr_valid = false;
        const hipError_t e = fault_due(ctx) ? hipErrorUnknown : hipMalloc(&ctx->lr_L, lbytes);
        if (e != hipSuccess) {
            ctx->lr_L = nullptr;
            quiesce(ctx);
            char msg[200];
            snprintf(msg, sizeof msg, "%s%zu bytes of factor (8 x rank %d x pitch %ld) could not be allocated: %s", who, lbytes, rank,
                     ctx->lda, hipGetErrorString(e));
            return fail(ctx, e == hipErrorOutOfMemory ? CGX_ERR_OOM : CGX_ERR_HIP, msg);
        }
        ctx->lr_L_rank = rank;
    }
    if (!ctx->lr_block) {
        ctx->lr_valid = false;
        cgx::LrWork measure{};
        Carver c{nullptr};
        carve_lr(c, ctx->lda, n, &measure);
        CGX_TRY(ensure_side_block(ctx, &ctx->lr_block, &ctx->lr_block_bytes, c.bytes()));
    }
    if (ctx->lr_valid) return CGX_OK;
    const cgx::LrWork w = lr_work(ctx);
    HIP_TRY(ctx, hipMemsetAsync(ctx->lr_L, 0, lbytes, st));                                   // the pad rows
    HIP_TRY(ctx, hipMemsetAsync(w.head, 0x7f, sizeof(cgx::LrHead), st));                      // every int = kLrArmed
    HIP_TRY(ctx, hipMemsetAsync(w.C, 0, (size_t)cgx::kLrLd * cgx::kLrLd * sizeof(double), st));
    HIP_TRY(ctx, cgx::launch_lr_init(s.A, ctx->lda, n, w, st));
    for (int t = 0; t < rank; ++t) HIP_TRY(ctx, cgx::launch_lr_step(s.A, ctx->lda, n, t, ctx->lr_L, w, st));
    HIP_TRY(ctx, cgx::launch_lr_finish(ctx->lr_L, ctx->lda, n, rank, ctx->precond_shift, w, st));
    CGX_TRY(arm_jbad(ctx));
    int block = 2;   // the sweep works on one block of a power of two >= rank; rows and columns past the rank are not touched
    while (block < rank) block *= 2;
    HIP_TRY(ctx, cgx::launch_bj_invert(w.C, cgx::kLrLd, rank, block, ctx->d_jbad, st));
    cgx::LrHead h{};
    HIP_TRY(ctx, hipMemcpyAsync(&h, w.head, sizeof h, hipMemcpyDeviceToHost, st));
    int bad = -1;
    CGX_TRY(read_jbad(ctx, &bad));   // (synchronises: h has landed)
    char msg[240];
    if (h.bad_step != cgx::kLrArmed) {
        snprintf(msg, sizeof msg, "%sthe matrix is not positive definite: at step %d the largest remaining diagonal entry (row %d) is not "
                                  "finite and > 0", who, h.bad_step, h.bad_row);
        return fail(ctx, CGX_ERR_BAD_ARG, msg);
    }
    if (h.bad_row != cgx::kLrArmed) {
        snprintf(msg, sizeof msg, "%sthe matrix is not positive definite: at step 0 the diagonal entry of row %d is not finite and > 0", who,
                 h.bad_row);
        return fail(ctx, CGX_ERR_BAD_ARG, msg);
    }
    if (h.delta_bad) {
        snprintf(msg, sizeof msg, "%sthe shift %.17g (%s) is not finite and > 0", who, h.delta,
                 ctx->precond_shift > 0.0 ? "as set" : "the mean remaining diagonal after the last step");
        return fail(ctx, CGX_ERR_BAD_ARG, msg);
    }
    if (bad >= 0) {
        snprintf(msg, sizeof msg, "%sdelta I + L^T L (rank %d) could not be inverted: a pivot of its factorisation is not finite and > 0", who, rank);
        return fail(ctx, CGX_ERR_BAD_ARG, msg);
    }
    ctx->lr_delta = h.delta;
    ctx->lr_valid = true;
    return CGX_OK;
}

cgx_status prepare_multi_precond(cgx_ctx *ctx, const std::string &fn)
{
    if (ctx->precond == CGX_PRECOND_JACOBI) {
        if (ctx->precond_block > 1)
            return fail(ctx, CGX_ERR_UNSUPPORTED, fn + ": block Jacobi (cgx_set_preconditioner_block > 1) has no multi-vector update kernel; "
                                                       "point Jacobi and CGX_PRECOND_PIVCHOL have");
        return prepare_jacobi(ctx);
    }
    if (ctx->precond == CGX_PRECOND_PIVCHOL) return prepare_lowrank(ctx);
    return fail(ctx, CGX_ERR_UNSUPPORTED, fn + ": unknown preconditioner");
}

}  // namespace cgxi
