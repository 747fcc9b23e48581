// cgx_multi_gemv.inc -- the body of the multi-vector K1, included into k_multi_gemv (cgx_multi.hip, PRE = false) and
// k_multi_gemv_pc (cgx_multi_pc.hip, PRE = true).  A text include, as cgx_symv_tiles.inc and cgx_p2p_update.inc: the plain kernels
// keep their code and registers exactly.  The including kernel provides W, FUSED, PRE and the names A, lda, n, nrhs, v (plain: the
// vectors; fused: p_old), p_new, r, rrp, g3, Y, partials, ms, k, tol, and rzp, mp (null constants where PRE is false).
//
// K1m shape: 8 waves per workgroup, each wave owns R consecutive rows, the workgroup 8R.  The workgroup sweeps the columns in
// chunks of kMultiChunk; the chunk of all W vectors is staged in LDS as [column j][kMultiChunk doubles], so that a lane's
// 16-B read of (j, c..c+1) is conflict free across the wave, and every lane streams its R rows of A with one 16-B load per row
// and 128-column step.  Every staged vector element serves the 8R rows of the workgroup; the A stream is the same as K1's.
// Per row and column the sum order is fixed (lane: ascending chunks and steps, .x then .y; wave: wave_sum_rows), and it does
// not depend on the column's position among the others, so permuting the columns permutes the results bit for bit.
//
// FUSED: iteration head, P = R + beta P_old staged (and stored once: chunk c by workgroup c mod grid), Y = A P, partials.
// Plain: Y = A V for the nrhs columns of V, partials of V_j . Y_j.  Y, partials and p_new are written for live columns only.
// PRE changes the head alone (multi_head, cgx_device.h); the vector the sweep calls r is then z = M^-1 r.
    constexpr int R = MultiShape<W>::R;
    constexpr int ROWS = kMultiWaves * R;
    constexpr int NV = R * W;
    __shared__ d2 tile[2][W][kMultiChunk / 2];
    __shared__ double red[kMultiWaves][NV];
    __shared__ double s_beta[W];
    __shared__ int s_live[W];

    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // wave-uniform: the row pointers live in SGPRs
    const int tid = threadIdx.x;

    if constexpr (FUSED) {
        for (int j = w; j < W; j += kMultiWaves) {
            double beta = 0.0;
            const bool live = j < nrhs && multi_head<PRE>(ms, mp, rzp, rrp, g3, j, k, tol, blockIdx.x == 0, &beta);
            if (lane == 0) { s_beta[j] = beta; s_live[j] = live ? 1 : 0; }
        }
    } else {
        if (tid < W) { s_beta[tid] = 0.0; s_live[tid] = tid < nrhs ? 1 : 0; }
    }
    __syncthreads();
    int any = 0;
#pragma unroll
    for (int j = 0; j < W; ++j) any |= s_live[j];
    if (FUSED && blockIdx.x == 0 && tid == 0 && !any && !ms->all_done) {
        ms->all_done = 1;                                   // the host polls this word
        ms->k_all = k - 1;
    }
    if (!any) return;                                       // every column has broken: the grid drains at once

    const long row_w = (long)blockIdx.x * ROWS + (long)w * R;
    const char *a_row[R];
#pragma unroll
    for (int i = 0; i < R; ++i) {
        long row = row_w + i;
        if (row > n - 1) row = n - 1;                       // tail workgroup: re-read the last row, result discarded
        a_row[i] = reinterpret_cast<const char *>(A + row * lda);
    }
    double acc[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) acc[i] = 0.0;

    const int ncols = (n + 1) & ~1;                         // pad columns up to lda are zero in A and in every vector
    const int nchunks = (ncols + kMultiChunk - 1) / kMultiChunk;
    constexpr int kStage = (W * kMultiChunk / 2 + kMultiThreads - 1) / kMultiThreads;   // 16-B pieces per thread and chunk
    d2 st[kStage];

    // the staged value of piece q of chunk c: (column j, 2 doubles); zero for a masked column and past n
    auto stage_load = [&](int c) {
#pragma unroll
        for (int u = 0; u < kStage; ++u) {
            const int q = tid + u * kMultiThreads;
            const int j = q / (kMultiChunk / 2), cc = q % (kMultiChunk / 2);
            const long col = (long)c * kMultiChunk + 2 * cc;
            d2 val = {0.0, 0.0};
            if (q < W * kMultiChunk / 2 && col < ncols && s_live[j]) {
                const long off = (long)j * lda + col;
                if constexpr (FUSED) {
                    const d2 po = *reinterpret_cast<const d2 *>(v + off);
                    const d2 rr = *reinterpret_cast<const d2 *>(r + off);
                    val.x = fma(s_beta[j], po.x, rr.x);     // cg.cc:127-129
                    val.y = fma(s_beta[j], po.y, rr.y);
                } else {
                    val = *reinterpret_cast<const d2 *>(v + off);
                }
            }
            st[u] = val;
        }
    };
    auto stage_store = [&](int c, int buf) {
        const bool owner = FUSED && (c % (int)gridDim.x) == (int)blockIdx.x;
#pragma unroll
        for (int u = 0; u < kStage; ++u) {
            const int q = tid + u * kMultiThreads;
            if (q < W * kMultiChunk / 2) {
                const int j = q / (kMultiChunk / 2), cc = q % (kMultiChunk / 2);
                tile[buf][j][cc] = st[u];
                const long col = (long)c * kMultiChunk + 2 * cc;
                if (owner && col < ncols && s_live[j]) *reinterpret_cast<d2 *>(p_new + (long)j * lda + col) = st[u];   // stored once
            }
        }
    };

    stage_load(0);
    stage_store(0, 0);
    __syncthreads();
    for (int c = 0; c < nchunks; ++c) {
        d2 a[kMultiSteps][R];
#pragma unroll
        for (int s = 0; s < kMultiSteps; ++s) {
            const int col = c * kMultiChunk + s * 128 + lane * 2;
            const unsigned off = (unsigned)(col < ncols ? col : 0) * 8u;
#pragma unroll
            for (int i = 0; i < R; ++i) {
                const d2 val = load_a<true>(reinterpret_cast<const double *>(a_row[i] + off));
                a[s][i] = col < ncols ? val : d2{0.0, 0.0};
            }
        }
        if (c + 1 < nchunks) stage_load(c + 1);
        const int buf = c & 1;
#pragma unroll
        for (int s = 0; s < kMultiSteps; ++s) {
#pragma unroll
            for (int j = 0; j < W; ++j) {
                const d2 p = tile[buf][j][s * 64 + lane];
#pragma unroll
                for (int i = 0; i < R; ++i) {
                    acc[i * W + j] = fma(a[s][i].x, p.x, acc[i * W + j]);
                    acc[i * W + j] = fma(a[s][i].y, p.y, acc[i * W + j]);
                }
            }
        }
        if (c + 1 < nchunks) stage_store(c + 1, buf ^ 1);
        __syncthreads();
    }

    // every lane group of 64 / NV lanes holds the total of one (row, column) pair
    const int vi = wave_sum_rows<NV>(acc, lane);
    const int i = vi / W, j = vi % W;
    const long row = row_w + i;
    double pv = 0.0;
    if ((lane & (64 / NV - 1)) == 0) {
        if (row < n && s_live[j]) {
            const double y = acc[0];
            Y[(long)j * lda + row] = y;
            const long off = (long)j * lda + row;
            const double pr = FUSED ? fma(s_beta[j], v[off], r[off]) : v[off];   // the p_j[row] this launch staged
            pv = pr * y;                                                          // cg.cc:105
        }
        red[w][vi] = pv;
    }
    __syncthreads();
    if (tid < W && s_live[tid]) {
        double s = 0.0;
        for (int ww = 0; ww < kMultiWaves; ++ww)
#pragma unroll
            for (int ii = 0; ii < R; ++ii) s += red[ww][ii * W + tid];
        partials[(long)tid * gridDim.x + blockIdx.x] = s;
    }
