// mpb_bgzf_lane.inc -- what ONE LANE of k_bgzf_deflate does (mpb_bgzf_kernels.hip), with no wave intrinsic in it, so that a host
// program runs the same text with checked loads (tests/helpers/bgzf_lane_check.cpp): the hash, the verified match, the greedy
// walk of one step, the token format and its widths, the length / distance code tables with their extra bits, the Huffman length
// builder with its limit, the canonical codes, the choice between a dynamic, a fixed and a stored block, the header writer and
// the bit writer.  The includer defines
//     BZ_FN                    the function qualifier (__device__ __forceinline__ / static inline)
//     BZ_LD8(text, i)          byte i of the member (the host's form checks 0 <= i < n)
//     BZ_LD64(text, i, n)      bytes i .. i + 7, little-endian, for i < n: the kernel's form is one unaligned 8-byte load that may
//                              run up to 7 bytes past n (its LDS array is longer than a member; what it reads there never reaches
//                              a result), the host's form loads the bytes below n checked and takes the others as 0
//     BZ_OR32(ptr, value)      *ptr |= value on a 32-bit word (the kernel's form is an LDS atomic OR: lanes share words)
// A member is at most MPB_BGZF_DATA bytes and is its own window: nothing here looks outside [0, n).

#define BZ_MIN_MATCH 3
#define BZ_MAX_MATCH 258
#define BZ_MAX_DIST  32768
#define BZ_HASH_BITS 14
#define BZ_HASH_SIZE (1 << BZ_HASH_BITS)
#define BZ_STEP      256                    // positions per step = lanes of the workgroup
#define BZ_NLL       288                    // literal/length symbols (286 used by a dynamic block; the fixed code names 288)
#define BZ_ND        32                     // distance symbols (30 used)
#define BZ_NCL       19
#define BZ_EOB       256
#define BZ_STORED    0
#define BZ_FIXED     1
#define BZ_DYNAMIC   2
#define BZ_TOK_LIT   0x80000000u            // token: 0 = the position starts none; BZ_TOK_LIT | byte; (len << 16) | (dist - 1)

// The two hash tables of a member, side by side in one array, one entry per bucket: table A over the next BZ_HA_BYTES bytes (short
// context), table B over the next BZ_HB_BYTES (long context: in a text over four letters the most recent place with the same
// few bytes is nearly always a useless one).  A position too close to the member's end for a table's context is not in that
// table (BZ_NO_HASH).  The values are measured ones: on the three renderings of tests/golden/test1.fastq.gz, contexts of 3 and
// 8 bytes with distance 1 alone gave 1.03 / 0.80 / 1.28 of zlib level 4's size (fastq / fasta / qual), 4 and 8 bytes with the
// distances 1..4 tried directly 0.98 / 0.76 / 1.05; one table over 3 bytes 1.53 / 2.26 / 2.07.  A match of exactly three bytes is
// then found at the short distances only.
#ifndef BZ_HA_BYTES
#define BZ_HA_BYTES 4
#endif
#ifndef BZ_HB_BYTES
#define BZ_HB_BYTES 8
#endif
#ifndef BZ_DIRECT
#define BZ_DIRECT 4                         // the distances 1 .. BZ_DIRECT are tried directly: closer than one step
#endif
#define BZ_NO_HASH 0xffffffffu
BZ_FN uint32_t bz_hash_at(const uint8_t *text, int n, int p, int bytes, uint32_t table)
{
    if (p + bytes > n) return BZ_NO_HASH;
    uint64_t v = BZ_LD64(text, p, n);
    if (bytes < 8) v &= (1ull << (8 * bytes)) - 1ull;
    return (uint32_t)((v * 0x9E3779B97F4A7C15ull) >> (64 - (BZ_HASH_BITS - 1))) + table * (BZ_HASH_SIZE / 2);
}
BZ_FN uint32_t bz_hash_a(const uint8_t *text, int n, int p) { return bz_hash_at(text, n, p, BZ_HA_BYTES, 0); }
BZ_FN uint32_t bz_hash_b(const uint8_t *text, int n, int p) { return bz_hash_at(text, n, p, BZ_HB_BYTES, 1); }

// bytes that agree between positions c < p, at most min(BZ_MAX_MATCH, n - p): every candidate is verified here, byte by byte
// (eight at a time: the first differing byte of two 8-byte words; a difference past the limit is cut off by it)
BZ_FN int bz_match_len(const uint8_t *text, int n, int c, int p)
{
    int lim = n - p;
    if (lim > BZ_MAX_MATCH) lim = BZ_MAX_MATCH;
    int l = 0;
    while (l < lim) {                                        // at most 33 trips
        const uint64_t x = BZ_LD64(text, c + l, n) ^ BZ_LD64(text, p + l, n);
        if (x) { l += __builtin_ctzll(x) >> 3; break; }
        l += 8;
    }
    return l < lim ? l : lim;
}

// The match of position p: cand_a / cand_b are what the two tables held for p BEFORE this step inserted (position + 1; 0:
// nothing), and the distances 1 .. BZ_DIRECT are tried directly (a run is closer than one step).  The longest wins, the first
// tried on a tie: the short distances, then the long context, then the short one.
BZ_FN void bz_find(const uint8_t *text, int n, int p, uint32_t cand_a, uint32_t cand_b, int *len_out, int *dist_out)
{
    int best = 0, dist = 0;
    if (p + BZ_MIN_MATCH <= n) {
        const int full = n - p < BZ_MAX_MATCH ? n - p : BZ_MAX_MATCH;      // a match of this length cannot be beaten
        for (int d = 1; d <= BZ_DIRECT && d <= p && best < full; d++) {
            const int l = bz_match_len(text, n, p - d, p);
            if (l >= BZ_MIN_MATCH && l > best) { best = l; dist = d; }
        }
        for (int k = 0; k < 2; k++) {
            const uint32_t cand = k ? cand_a : cand_b;
            if (cand == 0 || best >= full) continue;
            const int c = (int)cand - 1;
            if (c < 0 || c >= p || p - c > BZ_MAX_DIST || p - c <= BZ_DIRECT || p - c == dist) continue;
            const int l = bz_match_len(text, n, c, p);
            if (l >= BZ_MIN_MATCH && l > best) { best = l; dist = p - c; }
        }
    }
    *len_out = best; *dist_out = dist;
}

// The greedy parse of one step, by one lane: slen[k] is the match length at base + k (0: none), cnt the positions of the step,
// cur the first position no token covers yet.  Marks the token starts, returns the new cur (it may lie past the step).
BZ_FN int bz_walk_step(const uint16_t *slen, uint8_t *sflag, int base, int cnt, int cur)
{
    while (cur < base + cnt) {                               // at most cnt trips: cur grows by at least one
        const int k = cur - base;
        const int l = slen[k];
        sflag[k] = 1;
        cur += l ? l : 1;
    }
    return cur;
}

// ---- the code tables (RFC 1951 section 3.2.5), arithmetically --------------------------------------------------------------
BZ_FN void bz_len_code(int len, int *sym, int *ebits, int *eval)          // len 3..258
{
    const int l = len - 3;
    if (len == 258) { *sym = 285; *ebits = 0; *eval = 0; return; }
    if (l < 8) { *sym = 257 + l; *ebits = 0; *eval = 0; return; }
    const int nb = 31 - __builtin_clz((unsigned)l);         // 3..7
    const int e = nb - 2;
    *sym = 257 + 4 * (e + 1) + ((l >> e) & 3); *ebits = e; *eval = l & ((1 << e) - 1);
}
BZ_FN void bz_dist_code(int dist, int *sym, int *ebits, int *eval)        // dist 1..32768
{
    const int d = dist - 1;
    if (d < 4) { *sym = d; *ebits = 0; *eval = 0; return; }
    const int nb = 31 - __builtin_clz((unsigned)d);         // 2..14
    const int e = nb - 1;
    *sym = 2 * nb + ((d >> e) & 1); *ebits = e; *eval = d & ((1 << e) - 1);
}
BZ_FN int bz_len_extra(int sym) { return sym < 265 || sym >= 285 ? 0 : (sym - 261) >> 2; }
BZ_FN int bz_dist_extra(int sym) { return sym < 4 ? 0 : (sym >> 1) - 1; }

BZ_FN uint32_t bz_tok_literal(int byte) { return BZ_TOK_LIT | (uint32_t)byte; }
BZ_FN uint32_t bz_tok_match(int len, int dist) { return ((uint32_t)len << 16) | (uint32_t)(dist - 1); }

// ---- Huffman lengths with a limit ---------------------------------------------------------------------------------------------
// One lane.  The used symbols are sorted by (count, symbol), the tree is built with two queues, and when its depth exceeds `limit`
// every count is halved (rounding up, so none becomes 0) and the tree is built again: counts below 2^17 are all 1 after 17 rounds,
// and a tree of equal counts over m <= 288 symbols is 9 deep (5 for the 19 code-length symbols).  A code with fewer than two
// used symbols gets symbols added (count 1) until it has two, as zlib does: every tree written is complete (Kraft sum 1).
struct BzTree { uint32_t w[2 * BZ_NLL]; uint16_t par[2 * BZ_NLL]; uint16_t sym[BZ_NLL]; uint32_t f[BZ_NLL]; };

BZ_FN void bz_build_lengths(const uint32_t *freq, int nsym, int limit, uint8_t *len, BzTree *t)
{
    int m = 0;
    for (int s = 0; s < nsym; s++) {
        len[s] = 0;
        if (freq[s]) { t->sym[m] = (uint16_t)s; t->f[m] = freq[s]; m++; }
    }
    if (m == 0) { t->sym[0] = 0; t->f[0] = 1; t->sym[1] = 1; t->f[1] = 1; m = 2; }
    else if (m == 1) { t->sym[1] = (uint16_t)(t->sym[0] == 0 ? 1 : 0); t->f[1] = 1; m = 2; }
    for (int round = 0; round < 24; round++) {
        for (int i = 1; i < m; i++) {                        // insertion sort by (count, symbol); nearly sorted after a halving
            const uint32_t fi = t->f[i]; const uint16_t si = t->sym[i];
            int j = i;
            while (j > 0 && (t->f[j - 1] > fi || (t->f[j - 1] == fi && t->sym[j - 1] > si))) {
                t->f[j] = t->f[j - 1]; t->sym[j] = t->sym[j - 1]; j--;
            }
            t->f[j] = fi; t->sym[j] = si;
        }
        for (int i = 0; i < m; i++) t->w[i] = t->f[i];
        int li = 0, ii = m, nn = m;                          // next leaf, next internal node, nodes so far
        for (int k = 0; k < m - 1; k++) {
            int a, b;
            if (li < m && (ii >= nn || t->w[li] <= t->w[ii])) a = li++; else a = ii++;
            if (li < m && (ii >= nn || t->w[li] <= t->w[ii])) b = li++; else b = ii++;
            t->w[nn] = t->w[a] + t->w[b];
            t->par[a] = (uint16_t)nn; t->par[b] = (uint16_t)nn;
            nn++;
        }
        t->w[nn - 1] = 0;                                    // the root's depth; w becomes the depths (a parent lies above its children)
        int deepest = 0;
        for (int v = nn - 2; v >= 0; v--) {
            t->w[v] = t->w[t->par[v]] + 1;
            if (v < m && (int)t->w[v] > deepest) deepest = (int)t->w[v];
        }
        if (deepest <= limit) break;
        for (int i = 0; i < m; i++) t->f[i] = round >= 20 ? 1u : (t->f[i] + 1) >> 1;
    }
    for (int i = 0; i < m; i++) len[t->sym[i]] = (uint8_t)t->w[i];
}

// canonical codes from the lengths, bit-reversed: deflate packs a Huffman code from its most significant bit
BZ_FN void bz_make_codes(const uint8_t *len, int nsym, uint16_t *code)
{
    uint32_t count[16], next[16];
    for (int b = 0; b < 16; b++) count[b] = 0;
    for (int s = 0; s < nsym; s++) count[len[s]]++;
    count[0] = 0;
    uint32_t c = 0;
    next[0] = 0;
    for (int b = 1; b < 16; b++) { c = (c + count[b - 1]) << 1; next[b] = c; }
    for (int s = 0; s < nsym; s++) {
        const int l = len[s];
        uint32_t v = 0;
        if (l) {
            const uint32_t x = next[l]++;
            for (int b = 0; b < l; b++) v |= ((x >> b) & 1u) << (l - 1 - b);
        }
        code[s] = (uint16_t)v;
    }
}

// ---- the bit writer: value's low nbits (<= 32) at bit position pos of the word array, least significant bit first ---------------
BZ_FN void bz_put(uint32_t *words, uint32_t pos, uint32_t value, int nbits)
{
    if (nbits <= 0) return;
    const uint64_t v = (uint64_t)value << (pos & 31u);
    const uint32_t w = pos >> 5;
    BZ_OR32(&words[w], (uint32_t)v);
    if ((uint32_t)(v >> 32)) BZ_OR32(&words[w + 1], (uint32_t)(v >> 32));
}

// ---- the coder of one member --------------------------------------------------------------------------------------------------
struct BzCoder {
    uint32_t ll_freq[BZ_NLL], d_freq[BZ_ND], cl_freq[BZ_NCL];
    uint16_t ll_code[BZ_NLL], d_code[BZ_ND], cl_code[BZ_NCL];
    uint8_t ll_len[BZ_NLL], d_len[BZ_ND], cl_len[BZ_NCL];
    int32_t btype, hlit, hdist;
    uint32_t hdr_bits, total_bits;                           // of the block as it will be written (stored: 8 (n + 5))
    uint32_t n_lit, n_match, matched;                        // tokens of the member: literals, matches, bytes the matches cover
    BzTree tree;
};

BZ_FN void bz_fixed_lengths(uint8_t *ll_len, uint8_t *d_len)
{
    for (int s = 0; s < BZ_NLL; s++) ll_len[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8);
    for (int s = 0; s < BZ_ND; s++) d_len[s] = 5;
}

// bits of a token under the coder's final tables (0 for no token): a literal, or length code + extra, distance code + extra
BZ_FN int bz_token_bits(const BzCoder *cd, uint32_t tok)
{
    if (tok == 0) return 0;
    if (tok & BZ_TOK_LIT) return cd->ll_len[tok & 0xffu];
    int ls, le, lv, ds, de, dv;
    bz_len_code((int)(tok >> 16), &ls, &le, &lv);
    bz_dist_code((int)(tok & 0xffffu) + 1, &ds, &de, &dv);
    return cd->ll_len[ls] + le + cd->d_len[ds] + de;
}

BZ_FN void bz_emit_token(const BzCoder *cd, uint32_t *words, uint32_t pos, uint32_t tok)
{
    if (tok == 0) return;
    if (tok & BZ_TOK_LIT) { bz_put(words, pos, cd->ll_code[tok & 0xffu], cd->ll_len[tok & 0xffu]); return; }
    int ls, le, lv, ds, de, dv;
    bz_len_code((int)(tok >> 16), &ls, &le, &lv);
    bz_dist_code((int)(tok & 0xffffu) + 1, &ds, &de, &dv);
    bz_put(words, pos, (uint32_t)cd->ll_code[ls] | ((uint32_t)lv << cd->ll_len[ls]), cd->ll_len[ls] + le);      // <= 20 bits
    pos += (uint32_t)(cd->ll_len[ls] + le);
    bz_put(words, pos, (uint32_t)cd->d_code[ds] | ((uint32_t)dv << cd->d_len[ds]), cd->d_len[ds] + de);         // <= 28 bits
}

// The plan of the member's one block, by one lane, from the token histograms (ll_freq[BZ_EOB] is set here).  The dynamic header
// is written WITHOUT the repeat codes 16, 17 and 18 (valid deflate; every length goes out as its own code-length symbol), and all
// 19 code-length lengths are sent.  Whichever of dynamic, fixed and stored is shortest is chosen (stored, then fixed, on a tie),
// and the coder's tables are those of the choice when it returns.
BZ_FN void bz_plan_block(BzCoder *cd, int n)
{
    cd->ll_freq[BZ_EOB] = 1;
    uint8_t *ll = cd->ll_len, *dl = cd->d_len;
    bz_build_lengths(cd->ll_freq, 286, 15, ll, &cd->tree);
    ll[286] = 0; ll[287] = 0;
    bz_build_lengths(cd->d_freq, 30, 15, dl, &cd->tree);
    dl[30] = 0; dl[31] = 0;
    int hlit = 286, hdist = 30;
    while (hlit > 257 && ll[hlit - 1] == 0) hlit--;
    while (hdist > 1 && dl[hdist - 1] == 0) hdist--;
    for (int s = 0; s < BZ_NCL; s++) cd->cl_freq[s] = 0;
    for (int s = 0; s < hlit; s++) cd->cl_freq[ll[s]]++;
    for (int s = 0; s < hdist; s++) cd->cl_freq[dl[s]]++;
    bz_build_lengths(cd->cl_freq, 16, 7, cd->cl_len, &cd->tree);
    cd->cl_len[16] = 0; cd->cl_len[17] = 0; cd->cl_len[18] = 0;
    uint32_t hdr = 3 + 5 + 5 + 4 + 3 * BZ_NCL;
    for (int s = 0; s < 16; s++) hdr += cd->cl_freq[s] * cd->cl_len[s];
    uint32_t dyn = hdr, fix = 3;
    for (int s = 0; s < 286; s++) {
        const uint32_t f = cd->ll_freq[s];
        const uint32_t x = (uint32_t)bz_len_extra(s);
        dyn += f * (ll[s] + x);
        fix += f * ((s < 144 ? 8u : s < 256 ? 9u : s < 280 ? 7u : 8u) + x);
    }
    for (int s = 0; s < 30; s++) {
        const uint32_t f = cd->d_freq[s];
        const uint32_t x = (uint32_t)bz_dist_extra(s);
        dyn += f * (dl[s] + x);
        fix += f * (5u + x);
    }
    const uint32_t stored = 8u * ((uint32_t)n + 5u);
    cd->hlit = hlit; cd->hdist = hdist;
    if (stored <= dyn && stored <= fix) { cd->btype = BZ_STORED; cd->hdr_bits = 0; cd->total_bits = stored; return; }
    if (fix <= dyn) {
        cd->btype = BZ_FIXED; cd->hdr_bits = 3; cd->total_bits = fix;
        bz_fixed_lengths(ll, dl);
    } else {
        cd->btype = BZ_DYNAMIC; cd->hdr_bits = hdr; cd->total_bits = dyn;
        bz_make_codes(cd->cl_len, BZ_NCL, cd->cl_code);
    }
    bz_make_codes(ll, BZ_NLL, cd->ll_code);
    bz_make_codes(dl, BZ_ND, cd->d_code);
}

// the block header of a fixed or dynamic block into zeroed words, by one lane: BFINAL = 1 (a member is one block), BTYPE, and for
// a dynamic block HLIT, HDIST, HCLEN = 15, the 19 code-length lengths in the format's order, then hlit + hdist lengths
BZ_FN void bz_write_header(const BzCoder *cd, uint32_t *words)
{
    uint32_t pos = 0;
    bz_put(words, pos, 1u | ((uint32_t)cd->btype << 1), 3); pos += 3;
    if (cd->btype != BZ_DYNAMIC) return;
    bz_put(words, pos, (uint32_t)(cd->hlit - 257), 5); pos += 5;
    bz_put(words, pos, (uint32_t)(cd->hdist - 1), 5); pos += 5;
    bz_put(words, pos, (uint32_t)(BZ_NCL - 4), 4); pos += 4;
    for (int k = 0; k < BZ_NCL; k++) {                       // 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
        int s;
        switch (k) {
        case 0: s = 16; break; case 1: s = 17; break; case 2: s = 18; break; case 3: s = 0; break; case 4: s = 8; break;
        case 5: s = 7; break; case 6: s = 9; break; case 7: s = 6; break; case 8: s = 10; break; case 9: s = 5; break;
        case 10: s = 11; break; case 11: s = 4; break; case 12: s = 12; break; case 13: s = 3; break; case 14: s = 13; break;
        case 15: s = 2; break; case 16: s = 14; break; case 17: s = 1; break; default: s = 15; break;
        }
        bz_put(words, pos, cd->cl_len[s], 3); pos += 3;
    }
    for (int s = 0; s < cd->hlit; s++) { bz_put(words, pos, cd->cl_code[cd->ll_len[s]], cd->cl_len[cd->ll_len[s]]); pos += cd->cl_len[cd->ll_len[s]]; }
    for (int s = 0; s < cd->hdist; s++) { bz_put(words, pos, cd->cl_code[cd->d_len[s]], cd->cl_len[cd->d_len[s]]); pos += cd->cl_len[cd->d_len[s]]; }
}
