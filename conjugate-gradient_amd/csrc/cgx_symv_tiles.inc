// cgx_symv_tiles.inc -- the body of the symmetric tile kernel, included into k_symv_tiles (PRE = false) and k_pcg_symv_tiles (the
// Jacobi form, PRE = true).  A text include, as cgx_p2p_update.inc: the plain kernels keep their code and registers exactly.
// Expects B, FUSED, PRE and the kernels' parameters in scope.
    constexpr int H = B / 128;     // 1-KiB column pieces per row of a tile
    constexpr int R = 16 / H;      // rows per batch
    constexpr int RW = B / 4;      // rows per wave per tile
    static_assert(H >= 1 && RW % R == 0 && RW <= 64, "tile shape");
    __shared__ double rowbuf[2][B];
    __shared__ double colbuf[2][4][B];

    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long G = gridDim.x;
    const long t0 = tiles * (long)blockIdx.x / G, t1 = tiles * ((long)blockIdx.x + 1) / G;
    double beta = 0.0;
    if constexpr (FUSED) {
        const HeadLoadsOf<PRE> hl = head_issue_t<PRE>(sc, sv, k);
        const IterHead h = head_finish_t<PRE>(hl, sc, sv, k, tol);
        if (hl.done || h.stop) return;   // uniform over the grid: nothing is stored
        beta = h.beta;
    }
    if (t0 >= t1) return;
    long I, J;
    tri_tile(t0, nb, &I, &J);
    const double *rfull = sv.base;   // FUSED: the replicated r, contiguous and zero padded up to lda

    // the vector at the column pair (c, c+1) / at row i; exactly 0 from ncols / n on (and never read there)
    auto vec2 = [&](int c) {
        const bool ok = c < ncols;
        const int cc = ok ? c : 0;
        d2 p = *reinterpret_cast<const d2 *>(v + cc);
        if constexpr (FUSED) {
            const d2 r = *reinterpret_cast<const d2 *>(rfull + cc);
            p.x = fma(beta, p.x, r.x);                                   // cg.cc:127-129, the bits K1 stores
            p.y = fma(beta, p.y, r.y);
        }
        p.x = ok ? p.x : 0.0;
        p.y = ok ? p.y : 0.0;
        return p;
    };
    auto vec1 = [&](int i) {
        const bool ok = i < n;
        const int ii = ok ? i : 0;
        double p = v[ii];
        if constexpr (FUSED) p = fma(beta, p, rfull[ii]);
        return ok ? p : 0.0;
    };

    int buf = 0;
    for (long t = t0; t < t1; ++t) {
        const int r0 = (int)(I * B), c0 = (int)(J * B);
        const bool diag = I == J;
        int col[H];
        d2 pj[H];
#pragma unroll
        for (int h = 0; h < H; ++h) {
            col[h] = c0 + h * 128 + 2 * lane;
            pj[h] = vec2(col[h]);
            if constexpr (FUSED)   // p_new of block J is stored once: by wave 0 of the diagonal tile
                if (diag && w == 0 && col[h] < ncols) *reinterpret_cast<d2 *>(p_new + col[h]) = pj[h];
            if (col[h] >= ncols) col[h] = ncols - 2;   // clamped address; pj = 0 there and the column is never stored
        }
        const double pi_l = vec1(r0 + w * RW + (lane & (RW - 1)));   // p of the wave's row (lane & (RW-1)), 0 from n on
        d2 cacc[H];
#pragma unroll
        for (int h = 0; h < H; ++h) cacc[h] = d2{0.0, 0.0};

        for (int b = 0; b < RW / R; ++b) {
            const int rb = r0 + w * RW + b * R;
            d2 a[R][H];
#pragma unroll
            for (int q = 0; q < R; ++q) {
                long row = rb + q;
                if (row > n - 1) row = n - 1;   // rows from n on: the last row again, with p = 0 and no row store
                const char *ar = reinterpret_cast<const char *>(A + row * lda);
#pragma unroll
                for (int h = 0; h < H; ++h) a[q][h] = load_a<true>(reinterpret_cast<const double *>(ar + (unsigned)col[h] * 8u));
            }
            __builtin_amdgcn_sched_barrier(0);   // all of the batch's loads in flight before the first FMA
            double racc[R];
#pragma unroll
            for (int q = 0; q < R; ++q) {
                racc[q] = fma(a[q][0].y, pj[0].y, a[q][0].x * pj[0].x);
#pragma unroll
                for (int h = 1; h < H; ++h) racc[q] = fma(a[q][h].y, pj[h].y, fma(a[q][h].x, pj[h].x, racc[q]));
                const int src = b * R + q;   // wave-uniform
                const double pr = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(pi_l), src),
                                                   __builtin_amdgcn_readlane(__double2loint(pi_l), src));
#pragma unroll
                for (int h = 0; h < H; ++h) {
                    cacc[h].x = fma(a[q][h].x, pr, cacc[h].x);
                    cacc[h].y = fma(a[q][h].y, pr, cacc[h].y);
                }
            }
            const int myrow = wave_sum_rows<R>(racc, lane);
            if ((lane & (64 / R - 1)) == 0) rowbuf[buf][w * RW + b * R + myrow] = racc[0];
        }
        if (!diag)
#pragma unroll
            for (int h = 0; h < H; ++h) *reinterpret_cast<d2 *>(&colbuf[buf][w][h * 128 + 2 * lane]) = cacc[h];
        __syncthreads();
        for (int e = threadIdx.x; e < B; e += 256) {
            if (r0 + e < n) parts[J * lda + r0 + e] = rowbuf[buf][e];                                    // slot J of block I
            if (!diag && c0 + e < n)
                parts[I * lda + c0 + e] = ((colbuf[buf][0][e] + colbuf[buf][1][e]) + colbuf[buf][2][e]) + colbuf[buf][3][e];   // slot I of block J
        }
        buf ^= 1;
        if (++J == nb) { ++I; J = I; }
    }
