{
    // seg / wave_count: the reads this pass cannot finish.  A wave appends them to a segment of its own -- wave gw owns the
    // slots of the row blocks it walks, which start at 64 * (blocks owned by the waves before it) -- and leaves its count in
    // wave_count[gw]: no atomic (a returned atomic would drain the prefetch stream: vmcnt counts everything), and a list whose
    // order does not depend on timing.  k_nar_compact then makes the dense list.
    static_assert(D >= 2 && D <= 4, "ring depth");
    __shared__ nar_entry_t s_p[256];
    // one array per ring slot: a read of slot k is then provably independent of a DMA into slot k + 1 (the compiler orders
    // LDS reads behind LDS-DMA by what may alias)
    __shared__ __attribute__((aligned(16))) uint8_t s_ring0[4][MPB_NAR_PANEL];
    __shared__ __attribute__((aligned(16))) uint8_t s_ring1[4][MPB_NAR_PANEL];
    __shared__ __attribute__((aligned(16))) uint8_t s_ring2[D > 2 ? 4 : 1][D > 2 ? MPB_NAR_PANEL : 16];
    __shared__ __attribute__((aligned(16))) uint8_t s_ring3[D > 3 ? 4 : 1][D > 3 ? MPB_NAR_PANEL : 16];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    nar_stage_table(s_p, lut_g, tid);
    const int64_t nblk = (n + 63) >> 6;                       // row blocks of 64 reads
    const int ncq = (li + 63) >> 6;                           // 64-byte panels per row block (li >= 1)
    const int64_t gw = (int64_t)blockIdx.x * 4 + w, W = (int64_t)gridDim.x * 4;
    if (gw >= nblk) {
        if (lane == 0) wave_count[gw] = 0;
        return;
    }
    const int64_t total = ((nblk - gw + W - 1) / W) * ncq;    // panels this wave walks
    int32_t *const my_seg = seg + 64 * (gw * (nblk / W) + min(gw, nblk % W));
    int nlist = 0;                                            // wave-uniform
    const int r16 = lane & 15, cl = lane >> 4;
    const int row_chunks = __builtin_amdgcn_readfirstlane((int)(stride >> 4));
    uint32_t voff[4];
#pragma unroll
    for (int rg = 0; rg < 4; rg++) voff[rg] = (uint32_t)((rg * 16 + r16) * (int)stride + cl * 16);
    uint8_t *const ring[4] = {s_ring0[w], s_ring1[w], s_ring2[D > 2 ? w : 0], s_ring3[D > 3 ? w : 0]};
    const uint32_t ring_lds[4] = {lds_offset(s_ring0[w]), lds_offset(s_ring1[w]), lds_offset(s_ring2[D > 2 ? w : 0]),
                                  lds_offset(s_ring3[D > 3 ? w : 0])};

    // one panel = four DMA instructions, always four (the waits below count them)
    auto issue = [&](const int64_t b, const int c, const uint32_t slot) {
        const uint8_t *base = q + b * 64 * stride + c * 64;                        // wave-uniform
        const bool edge = (b * 64 + 64 > n) || (c * 4 + 4 > row_chunks);          // wave-uniform
        if (!edge) {
#pragma unroll
            for (int rg = 0; rg < 4; rg++) nar_dma16(base, voff[rg], slot + rg * 1024);
        } else {
            // last row block of the batch / last chunk column of a row whose stride is not a multiple of 64: rows and chunks
            // clamped into the matrix (what they deliver is never looked at)
            const int last_row = (int)(n - 1 - b * 64);                            // >= 0: the block holds at least one read
            const int ch = min(cl, row_chunks - 1 - c * 4);                        // >= 0: the panel starts inside the row
#pragma unroll
            for (int rg = 0; rg < 4; rg++)
                nar_dma16(base, (uint32_t)(min(rg * 16 + r16, last_row) * (int)stride + ch * 16), slot + rg * 1024);
        }
    };

    int64_t pf_b = gw, cur_b = gw;            // row block of the next panel to request / being computed
    int pf_c = 0, cur_c = 0;
    int64_t pf = 0;                           // panels requested so far
    auto request = [&](const uint32_t slot) {
        if (pf < total) {
            issue(pf_b, pf_c, slot);
            pf++;
            if (++pf_c == ncq) { pf_c = 0; pf_b += W; }
        }
    };
#pragma unroll
    for (int k = 0; k < D - 1; k++) request(ring_lds[k]);
    // A panel's slot is free as soon as its 64 bytes per lane are in registers -- at the START of its step, not at the end: the
    // request that refills it is made right behind those reads, so D panels are in flight while one is computed on, not D - 1
    // (what a CU can have in flight is what bounds the stream, and LDS capacity is what bounds that: profiles/r05_narrow_variants.txt).
    request(ring_lds[D - 1]);

    double v[R];
#pragma unroll
    for (int r = 0; r < R; r++) v[r] = r == 0 ? 1.0 : 0.0;
    const uint32_t tl = (uint32_t)((lane >> 4) * 1024 + (lane & 15) * 16);      // this lane's row inside a panel
    uint32_t nonzero = 0;

    auto step = [&](const int S, const int64_t s) {
        (void)s;
        // the panel of this step has landed when at most the requests made after it are still out
        const int64_t younger = pf - (s + 1);               // 0 .. D-1 panels (wave-uniform)
        {
        if (younger >= 3) nar_wait<12>();
        else if (younger == 2) nar_wait<8>();
        else if (younger == 1) nar_wait<4>();
        else nar_wait<0>();
        }
        // The lane's chunks of the panel -- all four, or (the last panel of a row whose length is no multiple of 64) those the read
        // reaches, the bytes past its end masked -- in registers; the slot is free then, and refilled before the run starts.
        const uint8_t *mine = ring[S] + tl;
        const int nbases = min(64, li - cur_c * 64);        // wave-uniform
        nar_chunks<R, true, MPB_NAR_AR>(v, nonzero, s_p, [&](const int c) { return mine + c * 256; }, (nbases + 15) >> 4, nbases >> 4, nbases, [&] {
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            request(ring_lds[S]);
        });
        if (++cur_c == ncq) {
            const int64_t i = cur_b * 64 + lane;
            const bool valid = i < n;
            const NarRead r = nar_finish<MPB_NAR_AR>(v, nonzero, prm, valid, valid, li, i, my_seg, nlist, lane);
            if (r.done) {
                ee[i] = r.e;
                ns[i] = r.nsv;
                pass[i] = (uint8_t)(r.keep ? 1 : 0);
            }
            cur_c = 0;
            cur_b += W;
        }
    };
    for (int64_t s = 0; s < total; s += D) {
        step(0, s);
        if (D > 1 && s + 1 < total) step(1 % D, s + 1);
        if (D > 2 && s + 2 < total) step(2 % D, s + 2);
        if (D > 3 && s + 3 < total) step(3 % D, s + 3);
    }
    if (lane == 0) wave_count[gw] = nlist;
}
