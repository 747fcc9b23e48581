// cgx_precond.cpp -- the set-up of the Jacobi preconditioners, inside cgx_solve_begin: point Jacobi and
// block Jacobi (section 13).  Set-up code only: the loop's kernels take dinv / W as arguments (enqueue_iteration, cgx_solve.cpp).
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
        if (!s.dinv) {
            const size_t zbytes = (size_t)(s.rv.S + (s.rv.S - s.rv.Sr)) * sizeof(double);
            HIP_TRY(ctx, hipMalloc(&s.dinv, (size_t)ctx->lda * sizeof(double)));
            HIP_TRY(ctx, hipMalloc(&s.zbuf, zbytes));
            HIP_TRY(ctx, hipMemsetAsync(s.zbuf, 0, zbytes, st));
        }
        s.zv = s.rv;
        s.zv.base = s.zbuf;
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

}  // namespace cgxi
