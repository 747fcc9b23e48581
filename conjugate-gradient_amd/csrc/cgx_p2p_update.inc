// cgx_p2p_update.inc -- the body of the fused update kernels of cgx_p2p.hip, included into k_update_xr_p2p (PRE = false) and
// k_pcg_update_p2p (the Jacobi form, PRE = true).  A text include rather than a device function: wrapping the body in a function
// changes the plain kernels' registers (measured with -Rpass-analysis=kernel-resource-usage), and the plain forms keep theirs.
// Expects TAGGED, SELFTEST, PRE and the kernels' parameters in scope.
    __shared__ double lds[4];
    const int tid = threadIdx.x, P = mv.nranks, me = mv.rank;
    const unsigned tag = p2p_tag(epoch);
    int done = 0;
    double rsold = 0.0, r_i = 0.0, p_i = 0.0, x_i = 0.0, d_i = 0.0;
    double *zrow = nullptr;   // PRE: &z[i]
    // (an atomic load, not a volatile one: the compiler waits for a volatile load on the spot -- a whole memory round trip
    // at the top of the kernel with nothing else in flight, seen in the ISA)
    const int had_err = __hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int i = blockIdx.x * 256 + tid;   // global row
    const int li = i - row0;
    const bool in = i < n, own = in && li >= 0 && li < rows;
    if constexpr (!SELFTEST) {
        done = sc->done;
        rsold = sc->rs[parity_rs];
        if (in) r_i = rv.base[i];
        if constexpr (PRE) {
            if (in) d_i = sums[i];
            // z's row address goes into vector registers here: kept as a scalar pointer to the end of the kernel it was the
            // pair of SGPRs too many (2 spilled, in the kernel-resource-usage remarks)
            zrow = vals + i;
            asm volatile("" : "+v"(zrow));
        }
        if (own) { p_i = p_new[i]; x_i = x[li]; }
    }
    const int npairs = P * cpr;
    // the first (peer, chunk) pair of this workgroup: its loads go out with the ones above, ahead of the first wait
    int pr = blockIdx.x;
    ChunkItem it{};
    if (pr < npairs) it = chunk_fetch(pr, cpr, ap_src, split, part_stride, apv.Sr, p_new + row0, rows);   // uniform per workgroup
    // `done` is identical on every rank (r.r is bit-identical), so either all ranks exchange or none does
    if (__syncthreads_or(done | had_err)) return;
    while (pr < npairs) {
        if constexpr (TAGGED) {
            const double d = chunk_dot<4>(it.pp, it.a, lds);
            unsigned long long *out = tagged_slot(mv, it.peer, chan, epoch, me);
            {
                // A lane holds the pair of rows (2L, 2L+1) of its wave's 128 rows; transposed through the wave so that one
                // store instruction covers 64 consecutive elements = 1 KiB without holes (whole 64-byte requests instead of
                // half-masked ones): lane L stores element L, then element 64 + L.
                const int lane = tid & 63, src = lane >> 1;
                const bool odd = (lane & 1) != 0;
                const double x1 = __shfl(it.a.x, src, 64), y1 = __shfl(it.a.y, src, 64);
                const double x2 = __shfl(it.a.x, 32 + src, 64), y2 = __shfl(it.a.y, 32 + src, 64);
                const int row_a = it.row - 2 * lane + lane, row_b = row_a + 64;
                if (row_a < apv.Sr) tagged_store(out + 2 * row_a, odd ? y1 : x1, tag);
                if (row_b < apv.Sr) tagged_store(out + 2 * row_b, odd ? y2 : x2, tag);
            }
            if (tid == 0) tagged_store(out + 2 * (apv.Sr + it.c), d, tag);
        } else {
            chunk_publish(mv, chan, epoch, cpr, apv.Sr, it, lds);
        }
        pr += gridDim.x;
        if (pr < npairs) it = chunk_fetch(pr, cpr, ap_src, split, part_stride, apv.Sr, p_new + row0, rows);
    }
    double cs = 0.0, ap_i = 0.0;
    if constexpr (TAGGED) {
        // Every thread polls the two words of its own Ap element and -- the first P*cpr threads -- of one chunk partial,
        // both in the same loop: all four loads of a round are in flight together (one after the other, the first wave of
        // every workgroup paid two memory round trips where one does).
        int ok = 1;
        const unsigned long long *wa = nullptr, *wp = nullptr;
        if (in) {
            const int q = (P > 1) ? seg_owner(apv, i) : 0;
            wa = tagged_slot(mv, me, chan, epoch, q) + 2 * (i - q * apv.n_loc);
        }
        if (tid < npairs) {
            const int q = tid / cpr, c = tid - q * cpr;
            wp = tagged_slot(mv, me, chan, epoch, q) + 2 * (apv.Sr + c);
        }
        const unsigned long long *dummy = tagged_slot(mv, me, chan, epoch, 0);   // a mapped address for the loads nobody needs
        bool need_a = wa != nullptr, need_p = wp != nullptr;
        const long long t0 = wall_clock64();
        while (need_a || need_p) {
            const unsigned long long *pa = need_a ? wa : dummy, *pp = need_p ? wp : dummy;
            const unsigned long long a0 = __hip_atomic_load(pa, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            const unsigned long long a1 = __hip_atomic_load(pa + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            const unsigned long long p0 = __hip_atomic_load(pp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            const unsigned long long p1 = __hip_atomic_load(pp + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            if (need_a && (unsigned)(a0 >> 32) == tag && (unsigned)(a1 >> 32) == tag) {
                ap_i = __longlong_as_double((long long)((a0 & 0xffffffffull) | (a1 << 32)));
                need_a = false;
            }
            if (need_p && (unsigned)(p0 >> 32) == tag && (unsigned)(p1 >> 32) == tag) {
                cs = __longlong_as_double((long long)((p0 & 0xffffffffull) | (p1 << 32)));
                need_p = false;
            }
            if (!(need_a || need_p)) break;
            __builtin_amdgcn_s_sleep(2);
            if (wall_clock64() - t0 > timeout_ticks) {               // bounded: give up, tell the host
                ok = 0;
                atomicExch(err, 1);
                break;
            }
        }
        for (int f = tid + 256; f < npairs; f += 256) {              // more than 256 partials (n > 131072): the rest, same order
            const int q = f / cpr, c = f - q * cpr;
            cs += tagged_load(tagged_slot(mv, me, chan, epoch, q) + 2 * (apv.Sr + c), tag, timeout_ticks, err, &ok);
        }
        if (!__syncthreads_and(ok)) return;
    } else {
        if (!__syncthreads_and(chunk_wait_all(mv, epoch, npairs, timeout_ticks, err))) return;
        // the row's Ap element first, the partials behind it: both loads are in flight together (the other way round the
        // partial is consumed -- waited for -- before the Ap load is even issued: one more memory round trip for wave 0)
        if (in) {
            const int q = (P > 1) ? seg_owner(apv, i) : 0;
            ap_i = chunk_read_ap(mv, chan, epoch, q, i - q * apv.n_loc);
        }
        cs = chunk_read_partials(mv, chan, epoch, cpr, apv.Sr, npairs);
    }
    const double conj = block_sum<4>(cs, lds);                       // bit-identical on every rank (cg.cc:106)
    if constexpr (SELFTEST) {
        if (in) vals[i] = ap_i;
        if (tid == 0) sums[blockIdx.x] = conj;
    } else if constexpr (PRE) {
        const double alpha = safeguarded_alpha(rsold, conj);         // alpha = rho / p.Ap, rho = r.z
        double rr = 0.0, rz = 0.0;
        if (in) {
            const PcRow o = pc_update_row(alpha, ap_i, r_i, d_i);
            rv.base[i] = o.r;
            *zrow = o.z;
            rr = o.rr;
            rz = o.rz;
        }
        if (own) x[li] = fma(alpha, p_i, x_i);
        rr = block_sum<4>(rr, lds);
        rz = block_sum<4>(rz, lds);
        if (tid == 0) {   // z + rv.Sr + wg and z + rv.S + wg, as pc_store_partials (here i = 256 wg)
            zrow[rv.Sr + (int)blockIdx.x - i] = rz;
            zrow[rv.S + (int)blockIdx.x - i] = rr;
        }
    } else {
        const double alpha = safeguarded_alpha(rsold, conj);         // cg.cc:107
        double rr = 0.0;
        if (in) {
            const double rn = fma(-alpha, ap_i, r_i);                 // cg.cc:113
            rv.base[i] = rn;
            rr = rn * rn;                                             // cg.cc:116
        }
        if (own) x[li] = fma(alpha, p_i, x_i);                        // cg.cc:110
        rr = block_sum<4>(rr, lds);
        if (tid == 0) rv.base[rv.Sr + blockIdx.x] = rr;
    }
