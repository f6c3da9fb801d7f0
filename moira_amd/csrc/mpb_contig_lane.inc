// mpb_contig_lane.inc -- what ONE LANE of k_contig does (mpb_contig_kernels.hip): the checks of a pair descriptor, the layout of
// the pair's LDS block, the load of the two reads, one step of the skewed Needleman-Wunsch fill, the 3' fix-up scan, the traceback
// and the consensus column.  No wave intrinsic lives here: what a lane gets from its neighbour is an argument, and the two wave
// operations of the kernel (the maximum over the lanes' scan keys, the prefix count of emitted columns) are its caller's.  The
// includer defines CD_FN (the function attributes) and cd_gload8 (one byte of a text buffer); tests/helpers/contig_device_check.cpp
// compiles the file on the host, runs 64 lane states in lockstep and checks every cd_gload8 against the buffer it may touch.
//
// The contract is byte identity with mct_contigs_from_fastq (contig.cpp): tie-break  left > max(diag, up) ? LEFT : (diag >= up ?
// DIAG : UP),  zero first row and column (pointing left / up), the last `>=` maximum of the last column and row (the column wins
// only on `>`), pointers on the last column / row rewritten, score = sum of the path's cells, and all of make_contig_impl.

#define CD_LANES 64
#define CD_MAX_LEN MPB_CONTIG_MAX_LEN
#define CD_DIAG 0
#define CD_UP 1
#define CD_LEFT 2

struct CdParams {
    int match, mismatch, gap, insert, deltaq, consensus, qcap, trim, offset;
    int maxabs;                              // max |match|, |mismatch|, |gap|
};

// lane l owns columns l * C + 1 .. (l + 1) * C of the reverse-complemented mate; nl lanes own a column.  A lane's pointers of
// one row are 2 bits per cell in a word of its own (pb bytes: no two lanes share a byte, so no LDS atomics are needed)
struct CdShape { int l1, l2, C, nl, pb, rowb; };
CD_FN CdShape cd_shape(int l1, int l2)
{
    CdShape s;
    s.l1 = l1; s.l2 = l2;
    s.C = (l2 + CD_LANES - 1) / CD_LANES;
    if (s.C < 1) s.C = 1;
    s.nl = (l2 + s.C - 1) / s.C;
    s.pb = s.C <= 4 ? 1 : 2;
    s.rowb = s.nl * s.pb;
    return s;
}

// byte offsets of the pair's LDS block (every piece on a 4-byte boundary)
struct CdLayout { int hdr, col, res, lastcol, lastrow, s1, s2, q1, q2, ptr, bytes; };
CD_FN int cd_r4(int x) { return (x + 3) & ~3; }
CD_FN CdLayout cd_layout(const CdShape &s)
{
    CdLayout L;
    int o = 0;
    L.hdr = o; o += 64;                                  // 16 ints the lanes share (lane 0 writes, all read)
    L.col = o; o += 4 * (s.l1 + s.l2);                   // one word per alignment column, in traceback order: i | j << 16 (0: a gap)
    L.res = o; o += 4 * (s.l1 + s.l2);                   // ... and what the consensus makes of it
    L.lastcol = o; o += cd_r4(2 * (s.l1 + 1));           // S(i, l2)
    L.lastrow = o; o += cd_r4(2 * (s.l2 + 1));           // S(l1, j)
    L.s1 = o; o += cd_r4(s.l1);
    L.s2 = o; o += cd_r4(s.l2);
    L.q1 = o; o += cd_r4(s.l1);
    L.q2 = o; o += cd_r4(s.l2);
    L.ptr = o; o += cd_r4(s.l1 * s.rowb);                // rows 1 .. l1 (row 0 and column 0 are implied)
    L.bytes = o;
    return L;
}
CD_FN int cd_lds_bytes(int l1, int l2) { return cd_layout(cd_shape(l1, l2)).bytes; }

// Every field of a descriptor against the buffers, before anything is derived from it.  Also what the device takes at all:
// 1 <= l1, l2 <= CD_MAX_LEN and the CPU's own 16-bit predicate.
CD_FN bool cd_row_ok(const mpb_pair_row &r, int64_t fbytes, int64_t rbytes, int64_t rec_cap, int maxabs)
{
    if (r.l1 < 1 || r.l1 > CD_MAX_LEN || r.l2 < 1 || r.l2 > CD_MAX_LEN) return false;
    if (r.hdr_len < 0 || (int64_t)r.hdr_len + 2 * ((int64_t)r.l1 + r.l2) > rec_cap) return false;
    if (r.fseq_off < 0 || r.fqual_off < 0 || r.fhdr_off < 0 || r.rseq_off < 0 || r.rqual_off < 0) return false;
    if (r.l1 > fbytes || r.fseq_off > fbytes - r.l1 || r.fqual_off > fbytes - r.l1) return false;
    if (r.hdr_len > fbytes || r.fhdr_off > fbytes - r.hdr_len) return false;
    if (r.l2 > rbytes || r.rseq_off > rbytes - r.l2 || r.rqual_off > rbytes - r.l2) return false;
    if ((int64_t)(r.l1 + r.l2 + 2) * maxabs >= 30000) return false;
    return true;
}

// ref: moira/moira.py:1210-1213 (complement_of in contig.cpp); 0: no complement
CD_FN int cd_complement(int b)
{
    switch (b) {
    case 'A': return 'T'; case 'C': return 'G'; case 'T': return 'A'; case 'G': return 'C';
    case 'N': return 'N'; case 'W': return 'W'; case 'S': return 'S'; case 'R': return 'Y';
    case 'Y': return 'R'; case 'M': return 'K'; case 'K': return 'M'; case 'B': return 'V';
    case 'V': return 'B'; case 'D': return 'H'; case 'H': return 'D'; case '-': return '-';
    case '.': return '.';
    default: return 0;
    }
}

// The lane's share of the two reads -> LDS: forward bases and qualities as they lie, the mate reverse-complemented with its
// qualities reversed.  false: the pair is handed back (a base without a complement, a quality below the offset, or a '-' in
// either read: make_contig takes a '-' of the alignment for a gap, so only the host can reproduce what such a read does).
CD_FN bool cd_load_lane(const mpb_pair_row &r, const uint8_t *ftext, const uint8_t *rtext, int offset, int lane,
                        uint8_t *s1, uint8_t *s2, uint8_t *q1, uint8_t *q2)
{
    bool ok = true;
    for (int k = lane; k < r.l1; k += CD_LANES) {
        const int b = cd_gload8(ftext + r.fseq_off + k), q = (int)cd_gload8(ftext + r.fqual_off + k) - offset;
        if (b == '-' || q < 0) ok = false;
        s1[k] = (uint8_t)b; q1[k] = (uint8_t)(q < 0 ? 0 : q);
    }
    for (int k = lane; k < r.l2; k += CD_LANES) {
        const int src = r.l2 - 1 - k;
        const int c = cd_complement(cd_gload8(rtext + r.rseq_off + src)), q = (int)cd_gload8(rtext + r.rqual_off + src) - offset;
        if (c == 0 || c == '-' || q < 0) ok = false;
        s2[k] = (uint8_t)c; q2[k] = (uint8_t)(q < 0 ? 0 : q);
    }
    return ok;
}

// ---- the fill ---------------------------------------------------------------------------------------------------------
// Rows are walked with a skew of one step per lane: at step t lane l computes row i = t - l + 1 of its C columns.  It keeps row
// i - 1 of them in registers (prev), gets S(i, l * C) -- its left border, which lane l - 1 computed one step earlier -- as
// `left_in`, and remembers the border of the row before (dleft) for the diagonal move.  Returns S(i, last column of the lane).
template <int C> struct CdLane { int prev[C]; int b[C]; int dleft; };

template <int C> CD_FN void cd_lane_init(CdLane<C> &st, const CdShape &sh, const uint8_t *s2, int lane)
{
#pragma unroll
    for (int c = 0; c < C; c++) {
        const int j = lane * C + 1 + c;
        st.prev[c] = 0;                                   // row 0
        st.b[c] = j <= sh.l2 ? s2[j - 1] : 0;
    }
    st.dleft = 0;
}

template <int C> CD_FN int cd_fill_step(CdLane<C> &st, const CdShape &sh, const CdParams &p, int lane, int t, int left_in,
                                        int out_prev, const uint8_t *s1, uint8_t *ptr, int16_t *lastcol, int16_t *lastrow)
{
    const int i = t - lane + 1;
    if (i < 1 || i > sh.l1 || lane >= sh.nl) return out_prev;
    const int a = s1[i - 1];
    int left = left_in, dg = st.dleft;
    unsigned bits = 0;
#pragma unroll
    for (int c = 0; c < C; c++) {
        const int j = lane * C + 1 + c;
        if (j <= sh.l2) {
            const int d = dg + (a == st.b[c] ? p.match : p.mismatch);
            const int u = st.prev[c] + p.gap;
            const int lf = left + p.gap;
            const int mx = d >= u ? d : u;
            const int v = lf > mx ? lf : mx;
            bits |= (unsigned)(lf > mx ? CD_LEFT : (d >= u ? CD_DIAG : CD_UP)) << (2 * c);
            dg = st.prev[c];
            st.prev[c] = v;
            left = v;
            if (j == sh.l2) lastcol[i] = (int16_t)v;
            if (i == sh.l1) lastrow[j] = (int16_t)v;
        }
    }
    st.dleft = left_in;
    if (sh.pb == 1) ptr[(i - 1) * sh.rowb + lane] = (uint8_t)bits;
    else ((uint16_t *)ptr)[(i - 1) * sh.nl + lane] = (uint16_t)bits;
    return left;
}
// steps of the fill: lane nl - 1 finishes row l1 at step l1 + nl - 2
CD_FN int cd_fill_steps(const CdShape &sh) { return sh.l1 + sh.nl - 1; }

template <int C> CD_FN int cd_ptr_at(const CdShape &sh, const uint8_t *ptr, int i, int j)       // 1 <= i <= l1, 1 <= j <= l2
{
    const int lane = (j - 1) / C, c = (j - 1) - lane * C;
    const unsigned w = sh.pb == 1 ? ptr[(i - 1) * sh.rowb + lane] : ((const uint16_t *)ptr)[(i - 1) * sh.nl + lane];
    return (int)((w >> (2 * c)) & 3u);
}

// ---- the 3' fix-up scan -----------------------------------------------------------------------------------------------
// A lane's candidates of a[0 .. n): key = (score + 32768) << 16 | index; the maximum key over all lanes is the LAST `>=`
// maximum (index 0 holds a score of 0, so the scan's sentinel of -10000 never wins).
CD_FN uint32_t cd_scan_key(const int16_t *a, int n, int lane)
{
    uint32_t best = 0;
    for (int k = lane; k < n; k += CD_LANES) {
        const uint32_t key = ((uint32_t)((int)a[k] + 32768) << 16) | (uint32_t)k;
        best = key > best ? key : best;
    }
    return best;
}
// 0: nothing to rewrite, 1: the last column above bci points up, 2: the last row right of bri points left
CD_FN int cd_fixup(const CdShape &sh, uint32_t colkey, uint32_t rowkey, int *bci, int *bri)
{
    const int cs = (int)(colkey >> 16) - 32768, rs = (int)(rowkey >> 16) - 32768;
    *bci = (int)(colkey & 0xffffu); *bri = (int)(rowkey & 0xffffu);
    if (*bci == sh.l1 && *bri == sh.l2) return 0;
    return cs > rs ? 1 : 2;
}

// ---- the traceback ----------------------------------------------------------------------------------------------------
// One lane walks it: at most l1 + l2 steps, then it stops.  col[r] = i | j << 16 of step r (0 where the read has a gap); the
// alignment's column k is col[K - 1 - k].  The score sums the path's cells as nw_align_diag does (border 0, last column / row
// kept, otherwise from the successor).  out[0] = K (-1: the walk did not end, the pair is handed back), out[1] = score,
// out[2..5] = first / last alignment column with a forward base, first / last with a reverse base.
template <int C> CD_FN void cd_traceback(const CdShape &sh, const CdParams &p, const uint8_t *s1, const uint8_t *s2,
                                         const uint8_t *ptr, const int16_t *lastcol, const int16_t *lastrow, int fix, int bci,
                                         int bri, uint32_t *col, int *out)
{
    int i = sh.l1, j = sh.l2, k = 0, score = 0, tracked = 0;
    int fi = -1, li = -1, fj = -1, lj = -1;              // in traceback order: first / last step that consumed a base
    const int bound = sh.l1 + sh.l2;
    for (int step = 0; step < bound && (i > 0 || j > 0); step++) {
        int pv;
        if (i == 0) pv = CD_LEFT;
        else if (j == 0) pv = CD_UP;
        else {
            pv = cd_ptr_at<C>(sh, ptr, i, j);
            if (fix == 1 && j == sh.l2 && i > bci) pv = CD_UP;
            if (fix == 2 && i == sh.l1 && j > bri) pv = CD_LEFT;
        }
        if (pv > CD_LEFT) break;
        const int here = (i == 0 || j == 0) ? 0 : (j == sh.l2 ? lastcol[i] : (i == sh.l1 ? lastrow[j] : tracked));
        score += here;
        const bool mv_i = pv != CD_LEFT, mv_j = pv != CD_UP;
        tracked = here - (pv == CD_DIAG ? (s1[i > 0 ? i - 1 : 0] == s2[j > 0 ? j - 1 : 0] ? p.match : p.mismatch) : p.gap);
        col[k] = (uint32_t)(mv_i ? i : 0) | ((uint32_t)(mv_j ? j : 0) << 16);
        if (mv_i) { if (fi < 0) fi = k; li = k; }
        if (mv_j) { if (fj < 0) fj = k; lj = k; }
        k++;
        if (mv_i) i--;
        if (mv_j) j--;
    }
    const bool done = i == 0 && j == 0 && fi >= 0 && fj >= 0;
    out[0] = done ? k : -1;
    out[1] = score;
    out[2] = k - 1 - li; out[3] = k - 1 - fi;            // fstart, fend
    out[4] = k - 1 - lj; out[5] = k - 1 - fj;            // rstart, rend
}

// ---- the consensus ----------------------------------------------------------------------------------------------------
// make_contig_impl's column k, from the column word cv: bit 0 a base is emitted, bit 1 a gap of the overlap, bit 2 a mismatch,
// bit 3 the quality does not fit its byte (the pair is handed back), bits 4-11 the base, bits 12-19 q + offset.
#define CD_EMIT 1u
#define CD_GAP 2u
#define CD_MISM 4u
#define CD_BAD 8u
CD_FN uint32_t cd_column(const CdParams &p, const uint8_t *s1, const uint8_t *s2, const uint8_t *q1, const uint8_t *q2,
                         const int32_t *tab_match, const int32_t *tab_mism, uint32_t cv, int k, int ostart, int oend, bool reversed)
{
    const int i = (int)(cv & 0xffffu), j = (int)(cv >> 16);
    const int fa = i ? s1[i - 1] : '-', ra = j ? s2[j - 1] : '-';
    const int fq = i ? q1[i - 1] : -1, rq = j ? q2[j - 1] : -1;
    const bool post = p.consensus == 2;
    uint32_t f = 0;
    int b = 0, q = 0;
    if (k < ostart) {
        if (!p.trim) { f = CD_EMIT; if (reversed) { b = ra; q = rq; } else { b = fa; q = fq; } }
    } else if (k > oend) {
        if (!p.trim) { f = CD_EMIT; if (reversed) { b = fa; q = fq; } else { b = ra; q = rq; } }
    } else if (fa == '-') {
        f = CD_GAP;
        if (post) { f |= CD_EMIT; b = 'N'; q = 2; }
        else if (rq > p.insert) { f |= CD_EMIT; b = ra; q = rq; }
    } else if (ra == '-') {
        f = CD_GAP;
        if (post) { f |= CD_EMIT; b = 'N'; q = 2; }
        else if (fq > p.insert) { f |= CD_EMIT; b = fa; q = fq; }
    } else if (fa == ra) {
        f = CD_EMIT; b = fa;
        if (p.consensus == 1) q = fq + rq;
        else if (post) q = tab_match[fq * 256 + rq];
        else q = fq >= rq ? fq : rq;
    } else {
        f = CD_EMIT | CD_MISM;
        if (!post) {
            const int d = fq - rq;
            if ((d < 0 ? -d : d) < p.deltaq) { b = 'N'; q = 2; }
            else if (fq >= rq) { b = fa; q = fq; }
            else { b = ra; q = rq; }
        } else if (fq == rq) { b = 'N'; q = 2; }
        else { b = fq > rq ? fa : ra; q = tab_mism[fq * 256 + rq]; }
    }
    if (!(f & CD_EMIT)) return f;
    if (p.qcap && !(q < p.qcap)) q = p.qcap;
    if (q < 0 || q + p.offset > 255) return f | CD_BAD;
    return f | ((uint32_t)(b & 255) << 4) | ((uint32_t)(q + p.offset) << 12);
}
