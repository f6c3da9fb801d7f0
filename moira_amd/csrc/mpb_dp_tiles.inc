// mpb_dp_tiles.inc -- the body of a DP class function: a run of consecutive tiles of one class, the tile walk (loads, prefetch,
// masking) and the end of a read, whatever the arithmetic.  mpb_kernels.hip includes it once per function that the kernels call
// (dp_tiles, dp_tiles_odds), each time with MPB_DP_AR naming the arithmetic: one text, and every function keeps a body of its own
// that the compiler sees exactly as if it had been written out (a shared inlined helper changes the exact bodies' register
// allocation: ODDS_MODE.md).  In scope: R, G, Ap, perm_cls, count, first_tile, n_tiles.
{
    const DpArgs &A = *Ap;
    constexpr int RPT = 64 / G;
    const int lane = lane_id();
    const int lig = lane & (G - 1);
    const bool leader = lig == 0;
    int keep = leader ? 0 : -1;
    asm volatile("" : "+v"(keep));        // opaque: keeps `& keep` a v_and (foldable into the DPP op), not a select
#pragma unroll 1
    for (int local_tile = first_tile; local_tile < first_tile + n_tiles; local_tile++) {
    const int slot = local_tile * RPT + lane / G;
    const bool valid = slot < count;
    const int idx = gload(perm_cls + (valid ? slot : count - 1));
    const int li = A.len ? clamp_len(gload(A.len + idx), A.prm.max_len) : A.prm.fixed_len;
    const uint8_t *row = A.q + (int64_t)idx * A.stride;

    int limax = li;                       // the longest read of the tile
    int nfull = li >> 4;                  // chunks that are complete in EVERY lane: no masking needed
    if (A.len) {                          // (fixed-length batches: every lane has the same li)
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            limax = max(limax, __shfl_xor(limax, off));
            nfull = min(nfull, __shfl_xor(nfull, off));
        }
    }
    limax = __builtin_amdgcn_readfirstlane(limax);  // wave-uniform trip counts
    nfull = __builtin_amdgcn_readfirstlane(nfull);
    const int nch = (limax + 15) >> 4;    // 16-byte chunks to walk

    double v[R];
#pragma unroll
    for (int r = 0; r < R; r++) v[r] = 0.0;
    if (leader) v[0] = 1.0;
    double p0 = 1.0;                      // ODDS: the product of the a's (row 0 of the reference's table); unused otherwise
    // ODDS, one lane per read: row 0 is the constant 1.  Opaque, so that row 1 keeps its fma (the compiler otherwise turns
    // fma(r, 1, w1) into an addition: the same rate, but the body then no longer reads as "one fused operation per cell")
    if (MPB_DP_AR == MPB_AR_ODDS && G == 1) asm volatile("" : "+v"(v[0]));

    // Each lane pulls its row 64 bytes at a time (4 x dwordx4, issued together, one 64-byte
    // segment of one line) and one super-chunk ahead of the arithmetic, so a cache line is
    // consumed while it is still resident instead of being re-fetched 16 bytes at a time.
    // A load is guarded by a WAVE-UNIFORM test only (the chunk lies inside the row: rows are `stride`
    // bytes whatever the read's length, and bytes past a read's end are masked below), so the
    // prefetch costs one 64-bit pointer bump per 64 bases instead of a compare / exec-mask / zero-fill
    // sequence per 16.
    const int row_chunks = __builtin_amdgcn_readfirstlane((int)(A.stride >> 4));
    const int nsc = (nch + 3) >> 2;                // wave-uniform 64-byte super-chunks
    const int nsc_fast = nfull >> 2;               // ... of which this many hold 64 valid bases in EVERY lane (all inside the row)
    uint4 cur[4], nxt[4];
#pragma unroll
    for (int p = 0; p < 4; p++) cur[p] = nxt[p] = make_uint4(0, 0, 0, 0);
    if (nsc_fast > 0) {
#pragma unroll
        for (int p = 0; p < 4; p++) cur[p] = gload16(row + p * 16);
        // Exactly four loads per trip, whatever the trip, issued BEFORE the trip's arithmetic and first
        // waited for at the top of the next trip: a whole super-chunk of FP64 work (1.5-6 us) covers the
        // memory latency.  The last trip has nothing new to fetch when the row ends here; it re-reads its
        // own (cache-resident) 64 bytes instead of branching, because a path-dependent load count makes
        // the compiler's wait-count bookkeeping fall back to "wait for everything" at once.
        // (Tried and rejected, bit-exact both: re-loading two chunks at a time into the registers just
        // consumed -- no second register set, no copies, but half the prefetch distance: k_dp +2 %.)
        for (int sc = 0; sc < nsc_fast; sc++) {
            const int nxt_sc = (sc * 4 + 8 <= row_chunks) ? sc + 1 : sc;     // scalar select
            const uint8_t *pf = row + (nxt_sc << 6);
#pragma unroll
            for (int p = 0; p < 4; p++) nxt[p] = gload16(pf + p * 16);
            // the machine scheduler otherwise sinks these loads to the end of the trip (their registers are
            // free there) and the next trip opens with vmcnt(0): the whole memory latency exposed
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int p = 0; p < 4; p++) dp_chunk<R, G, MPB_DP_AR>(v, p0, cur[p], keep);
#pragma unroll
            for (int p = 0; p < 4; p++) cur[p] = nxt[p];
        }
    }
    // tail: the super-chunks that are ragged in some lane (a 300-base read: bases 256..299)
    for (int sc = nsc_fast; sc < nsc; sc++) {
        if (!(sc > 0 && sc == nsc_fast && sc * 4 + 4 <= row_chunks)) {      // not already fetched by the loop above
#pragma unroll
            for (int p = 0; p < 4; p++) {
                cur[p] = make_uint4(0, 0, 0, 0);
                if (sc * 4 + p < row_chunks) cur[p] = gload16(row + (sc * 4 + p) * 16);   // wave-uniform guard
            }
        }
        const int pmax = min(4, nch - sc * 4);     // wave-uniform
#pragma unroll 1
        for (int p = 0; p < pmax; p++) {
            uint4 x = cur[0];
            cur[0] = cur[1]; cur[1] = cur[2]; cur[2] = cur[3];   // rotate: keeps every index static
            const int c = sc * 4 + p;
            int ndw = 4;                                 // dwords of this chunk to walk: wave-uniform
            if (c >= nfull) {                            // wave-uniform: only ragged tail chunks are masked
                const int nv = li - c * 16;              // may be <= 0 for reads shorter than the tile's longest
                x.x = mask_dword(x.x, nv); x.y = mask_dword(x.y, nv - 4);
                x.z = mask_dword(x.z, nv - 8); x.w = mask_dword(x.w, nv - 12);
                ndw = min(4, (limax - c * 16 + 3) >> 2); // a 300-base read ends 12 bases into its last chunk: 3 dwords, not 4
            }
            dp_chunk_tail<R, G, MPB_DP_AR>(v, p0, x, keep, ndw);
        }
    }

    // ---- epilogue: sequential CDF, first row above thr ----
    // ODDS: the registers hold the table divided by p0, so the CDF is compared with thr / p0 (the interpolation does not see
    // the scale).  Every w[j] <= prod (1 + r_k) = 1 / p0: while p0 >= 2^-900 nothing has overflowed and p0 is a normal number.
    // A read that fails the test (0 and NaN fail it too) is reported as one that never crossed: the overflow pass runs it.
    const double thr = MPB_DP_AR == MPB_AR_ODDS ? A.prm.thr / p0 : A.prm.thr;
    const bool in_range = MPB_DP_AR != MPB_AR_ODDS || p0 >= 0x1p-900;
    double lo = 0.0, hi = 0.0;
    int js = -1;
    bool writer;                                   // the lane that reports this read
    bool never_crossed = false;
    if (G == 1) {
        js = cdf_cross(v, 0.0, thr, 0, lo, hi);
        if (!in_range) js = -1;
        writer = valid;
        never_crossed = js < 0;
    } else {
        // Phase A: the running sum visits the G lanes of a read in order (same additions, same
        // order as the reference); a lane only notes whether the crossing falls inside its rows.
        // The CDF never decreases, so that is "sum after my rows > thr and nobody before me".
        double acc = 0.0, acc_in_mine = 0.0;
        int found = 0;
        bool mine = false;
#pragma unroll 1
        for (int g = 0; g < G; g++) {
            double acc_s = acc;
            int found_s = found;
            if (g > 0) {
                const int src = (lane & ~(G - 1)) + g - 1;
                acc_s = __shfl(acc, src);
                found_s = __shfl(found, src);
            }
            if (lig == g) {
                double a = acc_s;
#pragma unroll
                for (int r = 0; r < R; r++) a = a + v[r];
                const bool cross = !found_s && (a > thr);
                mine = cross;
                acc_in_mine = acc_s;
                acc = a;
                found = found_s | (cross ? 1 : 0);
            }
        }
        if (!in_range) { mine = false; found = 0; }         // (p0 is the same number in the G lanes of a read)
        // Phase B: only the crossing lane walks its rows again to pick out the two CDF values.
        if (mine) js = cdf_cross(v, acc_in_mine, thr, lig * R, lo, hi);
        never_crossed = (lig == G - 1) && !found;  // the last lane has seen the whole CDF
        writer = valid && (mine || never_crossed);
    }
    if (writer) {
        if (never_crossed && A.final_pass == 0) {
            const int pos = atomicAdd(A.ovf_count, 1);
            A.ovf_list[pos] = idx;
        } else if (never_crossed && A.final_pass == 2) {
            A.pass[idx] = 2;                                   // small-batch path: the host re-runs the batch
        } else {
            double e;
            if (MPB_DP_AR == MPB_AR_ODDS) e = cross_ee_odds(!never_crossed, js, A.prm.thr, p0, lo, hi);
            else e = cross_ee(!never_crossed, js, thr, lo, hi);
            const int nsv = A.perm_ns ? (int)gload(A.perm_ns + (perm_cls - A.perm) + slot) : gload(A.ns + idx);
            if ((A.prm.flags & MPB_FLAG_COUNT_CELLS) && !never_crossed) {      // diagnostic, off by default
                // the table the reference fills for this read: rows 0..js over the L' = len - Ns scored bases, of which
                // row j is non-zero from base j on: sum_k min(k + 1, J), J = js + 1 (SURVEY 8d "algorithmic flops")
                const int J = js + 1, Lp = li - nsv;                 // J <= 1024, Lp <= 16383: 32-bit arithmetic is enough
                const int cells = J <= Lp ? ((J * (J + 1)) >> 1) + (Lp - J) * J : (Lp * (Lp + 1)) >> 1;
                atomicAdd(&mpb_s_cells, (unsigned long long)(unsigned int)cells);
            }
            e = mpb_add_ns(A.prm, e, nsv);
            if (MPB_DP_AR != MPB_AR_EXACT && A.final_pass != 1 && !never_crossed) {
                // MPB_FLAG_FAST_FMA and MPB_FLAG_ODDS keep the DECISIONS exact: an ee that lands within 1e-9 relative of
                // the threshold (or, with --round, of an integer) is not trusted -- the read goes to the second
                // pass, which always runs the three-rounding arithmetic
                if (mode_unsure(A.prm, e, li)) {
                    if (A.final_pass == 0) { const int pos = atomicAdd(A.ovf_count, 1); A.ovf_list[pos] = idx; }
                    else A.pass[idx] = 2;
                    continue;
                }
            }
            const bool keep_read = mpb_round_and_keep(A.prm, e, class_has_n(A, idx), li);
            gstore(A.ee + idx, e);
            gstore(A.pass + idx, (uint8_t)(keep_read ? 1 : 0));
        }
    }
    }   // tiles of this run
}
