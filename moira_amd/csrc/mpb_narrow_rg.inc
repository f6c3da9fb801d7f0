{
    __shared__ nar_entry_t s_p[256];
    __shared__ __attribute__((aligned(128))) uint8_t s_tile[4][MPB_NRS_TILE];
    __shared__ uint32_t s_row[4][64];                         // byte offsets of the rows of the group being loaded, from its window's base
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    nar_stage_table(s_p, lut_g, tid);
    const int gw = blockIdx.x * 4 + w;
    const int ngroups = (int)((n + 63) >> 6), nwin = (int)((n + MPB_RG_WIN - 1) / MPB_RG_WIN), nwaves = (int)gridDim.x * 4;
    const int g0 = __builtin_amdgcn_readfirstlane(rg_first_group(wpre, gpre, nwin, ngroups, gw, nwaves, lane));
    const int g1 = __builtin_amdgcn_readfirstlane(rg_first_group(wpre, gpre, nwin, ngroups, gw + 1, nwaves, lane));
    if (lane == 0) gstart[gw] = g0;                           // (where the wave's list segment starts: k_nar_compact)
    if (g0 >= g1) {
        if (lane == 0) wave_count[gw] = 0;
        return;
    }
    int32_t *const my_seg = seg + 64 * (int64_t)g0;
    int nlist = 0;                                            // wave-uniform
    uint8_t *const tile = s_tile[w];
    const int istride = __builtin_amdgcn_readfirstlane((int)stride);
    const int r8 = lane >> 3, c8 = lane & 7;                  // stream 8 j + r8 of load instruction j: the lane's row
    int wr_even, wr_odd, x0;
    nar_tile_lane(lane, wr_even, wr_odd, x0);

    // a group's order entries {read, length}: -1 / -1 past the batch or past the wave's range; length -1: outside 0..max_len
    auto fetch = [&](const int g, int &idx, int &ln) {
        const int64_t p = (int64_t)g * 64 + lane;
        unsigned long long e = ~0ull;                           // {-1, -1}
        if (g < g1 && p < n) e = gload(reinterpret_cast<const unsigned long long *>(ord) + p);
        idx = (int)(uint32_t)e; ln = (int)(uint32_t)(e >> 32);
    };
    int cur_idx, cur_len, nx_idx, nx_len, nn_idx, nn_len;
    fetch(g0, cur_idx, cur_len);
    fetch(g0 + 1, nx_idx, nx_len);
    fetch(g0 + 2, nn_idx, nn_len);

    // arming a group for loading: per-lane row offsets from the window's base, the group's chunks (longest read) and the
    // chunks complete in every lane (shortest)
    uint32_t *const rows = s_row[w];
    const uint8_t *wbase = q;
    int ld_maxc = 0, ld_full = 0;
    auto arm = [&](const int g, const int idx, const int ln) {
        const int64_t wrow = ((int64_t)g * 64) & ~(int64_t)(MPB_RG_WIN - 1);          // first row of the group's window
        wbase = q + wrow * stride;
        const bool good = idx >= 0 && ln >= 0;
        const int rowoff = idx >= 0 ? (int)(idx - wrow) * istride : 0;                // (rows past the batch: the window's first)
        int mx = good ? (ln + 15) >> 4 : 0, mn = good ? ln >> 4 : 0x7fffffff;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) { mx = max(mx, __shfl_xor(mx, off)); mn = min(mn, __shfl_xor(mn, off)); }
        ld_maxc = __builtin_amdgcn_readfirstlane(mx);
        ld_full = __builtin_amdgcn_readfirstlane(mn);
        rows[lane] = (uint32_t)rowoff;                          // (the loads of the group before this one have all been issued)
    };
    u32x4 pre[8];
    auto load_panel = [&](const int pk) {
        const uint8_t *pb = wbase + pk * 128;                   // wave-uniform
        uint32_t voff[8];
#pragma unroll
        for (int j = 0; j < 8; j++) voff[j] = rows[8 * j + r8] + (uint32_t)(c8 * 16);
        if (8 * pk + c8 < ld_maxc) {                            // (the group's last panel: only the chunks its longest read has)
#pragma unroll
            for (int j = 0; j < 8; j++) pre[j] = *(const __attribute__((address_space(1))) u32x4 *)(pb + voff[j]);
        }
    };
    arm(g0, cur_idx, cur_len);
    int cur_maxc = ld_maxc, cur_full = ld_full;
    load_panel(0);

    double v[R];
#pragma unroll
    for (int r = 0; r < R; r++) v[r] = r == 0 ? 1.0 : 0.0;
    uint32_t nonzero = 0;

    for (int g = g0; g < g1; g++) {
        const int np = __builtin_amdgcn_readfirstlane(max(1, (cur_maxc + 7) >> 3));      // panels of this group
        for (int pk = 0; pk < np; pk++) {
            nar_tile_write(tile, wr_even, wr_odd, pre);
            nar_tile_fence();
            {
                int next_pk = pk + 1;
                const bool next_group = next_pk == np && g + 1 < g1;
                if (next_group) { arm(g + 1, nx_idx, nx_len); next_pk = 0; }
                if (next_pk < np || next_group) load_panel(next_pk);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const int cb = 8 * pk + 4 * h;                   // first chunk of this half
                const int rem = cur_maxc - cb;                   // chunks of the group's longest read from here on
                if (rem <= 0) continue;
                const int fullc = cur_full - cb;                 // ... that are complete in every lane
                const int nbl = cur_len - 16 * cb;               // this lane's bases from here on (may be <= 0)
                const auto chunk = [&](const int c) { return tile + (x0 ^ ((h * 4 + c) << 4)); };
                if (MPB_NAR_RLO < R && cur_maxc <= split) {               // a short group: rows 0 .. RLO-1 only (v[RLO ..] stay zero)
                    double (&vl)[MPB_NAR_RLO] = *reinterpret_cast<double (*)[MPB_NAR_RLO]>(&v[0]);
                    nar_chunks<MPB_NAR_RLO, false, MPB_NAR_AR>(vl, nonzero, s_p, chunk, rem >= 4 ? 4 : rem, fullc, nbl);
                } else {
                    nar_chunks<R, false, MPB_NAR_AR>(v, nonzero, s_p, chunk, rem >= 4 ? 4 : rem, fullc, nbl);
                }
            }
            nar_tile_fence();                                   // the tile is overwritten by the next panel
        }
        // ---- the group is done: nar_finish written out, with the lane's own length (and a length outside 0..max_len is handed back).
        // This kernel sits at its register cap: through the helper it needs a VGPR more at R = 2 and 4 more bytes of spill at R = 3, 4.
        {
            const int64_t i = cur_idx;
            const int li = cur_len;
            const bool valid = cur_idx >= 0, good = valid && li >= 0;
            double acc = 0.0, lo = 0.0, hi = 0.0;
            int js = -1;
#pragma unroll
            for (int r = 0; r < R; r++) {
                const double na = acc + v[r];
                const bool hit = (js < 0) && (na > prm.thr);
                lo = hit ? acc : lo;
                hi = hit ? na : hi;
                js = hit ? r : js;
                acc = na;
            }
            bool done = good && js >= 0;
            if (MPB_NAR_AR == MPB_AR_ODDS) {                                 // (the loop above is dead code in this form)
                const int nsv = li - (int)nonzero;
                double e = 0.0;
                bool keep = false;
                done = good && nar_odds_result(v, prm, nsv, li, e, keep);
                if (done) {
                    ee[i] = e;
                    ns[i] = nsv;
                    pass[i] = (uint8_t)(keep ? 1 : 0);
                }
            } else if (done) {
                const int nsv = li - (int)nonzero;                           // 'N' bases (a read with an 'n' never gets here)
                double e;
                const bool keep = read_result(prm, true, js, lo, hi, nsv, nsv > 0, li, e);
                ee[i] = e;
                ns[i] = nsv;
                pass[i] = (uint8_t)(keep ? 1 : 0);
            }
            const unsigned long long todo = __ballot(valid && !done);
            if (todo) {
                if (valid && !done) my_seg[nlist + __popcll(todo & ((1ull << lane) - 1ull))] = (int32_t)i;
                nlist += __popcll(todo);
            }
#pragma unroll
            for (int r = 0; r < R; r++) v[r] = r == 0 ? 1.0 : 0.0;
            nonzero = 0;
        }
        cur_idx = nx_idx; cur_len = nx_len;
        nx_idx = nn_idx; nx_len = nn_len;
        cur_maxc = __builtin_amdgcn_readfirstlane(ld_maxc); cur_full = __builtin_amdgcn_readfirstlane(ld_full);
        fetch(g + 3, nn_idx, nn_len);
    }
    if (lane == 0) wave_count[gw] = nlist;
}
