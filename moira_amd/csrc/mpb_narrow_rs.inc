{
    __shared__ nar_entry_t s_p[256];
    __shared__ __attribute__((aligned(128))) uint8_t s_tile[4][MPB_NRS_TILE];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    nar_stage_table(s_p, lut_g, tid);
    const int64_t rows_sb = 64 * (int64_t)k;                  // reads of a stream block: 64 lanes x k reads each
    const int64_t nsb = (n + rows_sb - 1) / rows_sb;
    const int KB = __builtin_amdgcn_readfirstlane((int)(k * stride));      // bytes of a lane's stream: a multiple of 128
    const int NP = KB >> 7;                                   // its panels
    const int istride = __builtin_amdgcn_readfirstlane((int)stride);
    const int64_t gw = (int64_t)blockIdx.x * 4 + w, W = (int64_t)gridDim.x * 4;
    if (gw >= nsb) {
        if (lane == 0) wave_count[gw] = 0;
        return;
    }
    const int64_t total = ((nsb - gw + W - 1) / W) * NP;      // panels this wave walks
    int32_t *const my_seg = seg + rows_sb * (gw * (nsb / W) + min(gw, nsb % W));
    int nlist = 0;                                            // wave-uniform
    uint8_t *const tile = s_tile[w];
    const int r8 = lane >> 3, c8 = lane & 7;                  // stream 8 j + r8 of load instruction j: the lane's slot c8 of panel bytes
    const int voff = r8 * KB + c8 * 16;
    int wr_even, wr_odd, x0;
    nar_tile_lane(lane, wr_even, wr_odd, x0);

    u32x4 pre[8];
    auto load_panel = [&](const int64_t sb, const int pk) {
        const uint64_t base = (uint64_t)(uintptr_t)q + (uint64_t)(sb * rows_sb) * (uint64_t)stride;
        const int64_t rows_here = (n - sb * rows_sb) < rows_sb ? (n - sb * rows_sb) : rows_sb;
        const uint32_t b_lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)base);
        const uint32_t b_hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(base >> 32));
        const uint32_t b_n = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(rows_here * stride));
        const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
            (void *)(uintptr_t)(((uint64_t)b_hi << 32) | b_lo), 0, (int)b_n, 0x00020000);
#pragma unroll
        for (int j = 0; j < 8; j++) pre[j] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff, j * 8 * KB + pk * 128, 0);
    };
    int64_t pf_sb = gw, cur_sb = gw;
    int pf_pk = 0, cur_pk = 0;
    load_panel(pf_sb, pf_pk);
    if (++pf_pk == NP) { pf_pk = 0; pf_sb += W; }

    double v[R];
#pragma unroll
    for (int r = 0; r < R; r++) v[r] = r == 0 ? 1.0 : 0.0;
    uint32_t nonzero = 0;
    int u = 0, sread = 0;                                      // position in the stream: byte u of its read number sread (wave-uniform)

    // ---- a read is done: nar_finish.  Two reads per lane: result arrays aligned for a lane's pair (R <= 3 only: with four rows the
    // held results do not fit the 128 registers of four waves per SIMD)
    const bool pair_stores = R <= 3 && k == 2 && (((uintptr_t)ee & 15) | ((uintptr_t)ns & 7) | ((uintptr_t)pass & 1)) == 0;
    double held_e = 0.0;
    int held_ns = 0;
    uint8_t held_ps = 0;
    bool held_ok = false;
    auto finish = [&](const int64_t sb, const int sr) {
        const int64_t i = sb * rows_sb + (int64_t)lane * k + sr;
        const NarRead r = nar_finish<MPB_NAR_AR>(v, nonzero, prm, i < n, i < n, li, i, my_seg, nlist, lane);
        if (r.done) {
            const double e = r.e;
            const int nsv = r.nsv;
            const uint8_t ps = (uint8_t)(r.keep ? 1 : 0);
            if (pair_stores && sr == 0) {
                // two reads per lane: the first one's results wait in registers for the second's, and go out together -- 16 + 8 + 2
                // contiguous bytes per lane instead of two half-used sectors a panel and a half apart (writes 0.26 -> 0.13 GB)
                held_e = e; held_ns = nsv; held_ps = ps;
            } else if (pair_stores && held_ok) {
                *reinterpret_cast<double2 *>(ee + i - 1) = make_double2(held_e, e);
                *reinterpret_cast<int2 *>(ns + i - 1) = make_int2(held_ns, nsv);
                *reinterpret_cast<uint16_t *>(pass + i - 1) = (uint16_t)(held_ps | ((uint16_t)ps << 8));
            } else {
                ee[i] = e;
                ns[i] = nsv;
                pass[i] = ps;
            }
        }
        if (pair_stores) {
            if (sr == 0) held_ok = r.done;
            else if (held_ok && !r.done) { ee[i - 1] = held_e; ns[i - 1] = held_ns; pass[i - 1] = held_ps; }   // the second one is handed back (or past the end)
        }
    };
    for (int64_t t = 0; t < total; t++) {
        // the panel requested one panel ago -> tile (the tile's last reads were issued before: LDS runs a wave's operations in order)
        nar_tile_write(tile, wr_even, wr_odd, pre);
        nar_tile_fence();
        if (t + 1 < total) {                                    // in flight while this panel is computed on
            load_panel(pf_sb, pf_pk);
            if (++pf_pk == NP) { pf_pk = 0; pf_sb += W; }
        }
        __builtin_amdgcn_sched_barrier(0);
        // ---- the panel's two 64-byte halves, four 16-byte chunks each.  The chunks of a half that belong to ONE read go through
        // one run (nar_chunks), so a 300-base read's last 44 bases take the same code as the others, as 48.  A read may end -- and the
        // next one begin -- anywhere a chunk does (strides that are no multiple of 64): then the half is several runs; row
        // padding is skipped by whole chunks.  All of it wave-uniform.
#pragma unroll
        for (int h = 0; h < 2; h++) {
            if (ALIGNED) {
                // rows of a multiple of 64 bytes: a read starts with a half, so a half holds chunks of ONE read -- one run, every
                // address a constant (the form measured in profiles/r05_narrow_variants.txt; the loop below costs it 2-3 %)
                const int nb = li - u;                          // bases of the current read from this half on
                if (nb > 0) {
                    nar_chunks<R, true, MPB_NAR_AR>(v, nonzero, s_p, [&](const int c) { return tile + (x0 ^ ((h * 4 + c) << 4)); }, nb >= 64 ? 4 : (nb + 15) >> 4, nb >> 4, nb);
                    if (nb <= 64) finish(cur_sb, sread);
                }
                u += 64;
                if (u == istride) { u = 0; sread++; }
                continue;
            }
            int p = 0;                                          // chunk of this half
            while (p < 4) {
                const int nb = li - u;                          // bases of the current read from here on
                if (nb <= 0) {                                  // its padding: on to the next read, or to the end of the half
                    const int skip = min((istride - u) >> 4, 4 - p);
                    p += skip;
                    u += 16 * skip;
                } else {
                    const int nch = min((nb + 15) >> 4, 4 - p); // chunks of this read in what is left of the half
                    const int c0 = h * 4 + p;
                    nar_chunks<R, true, MPB_NAR_AR>(v, nonzero, s_p, [&](const int c) { return tile + (x0 ^ ((c0 + c) << 4)); }, nch, nb >> 4, nb);
                    p += nch;
                    u += 16 * nch;
                    if (16 * nch >= nb) finish(cur_sb, sread);  // the read is done (u may stand in its padding now)
                }
                if (u >= istride) { u = 0; sread++; }
            }
        }
        if (++cur_pk == NP) { cur_pk = 0; cur_sb += W; sread = 0; }
        nar_tile_fence();                                       // the tile is overwritten by the next panel
    }
    if (lane == 0) wave_count[gw] = nlist;
}
