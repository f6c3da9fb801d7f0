// mpb_inflate_lane.inc -- what one lane of k_bgzf_inflate does (mpb_inflate_kernels.hip), and the order in which the 64 lanes of
// the member's wave do it (bi_member).  Included by the kernel unit and by tests/helpers/inflate_lane_check.cpp, which runs the
// same text on the host: 64 lane states in lockstep, every load of the compressed bytes checked.  The includer defines
//   BI_FN                      function qualifiers
//   BI_LD_IN16(in, q, w)       w[0..3] = the 16 bytes at in + q (q a multiple of 16; the caller has checked the range)
//   BI_LD_IN8(in, q)           the byte at in + q (range checked by the caller)
//   BI_ST_OUT16(text, q, w)    the 16 bytes at text + q (a 16-byte boundary of the text) = w[0..3]
//   BI_ST_OUT8(text, q, b)     the byte at text + q = b
//   BI_ATOMIC_INC(ptr)         *ptr += 1 on a uint32_t in the wave's shared memory, safe against the other lanes
//   BI_SYNC()                  shared-memory writes of all lanes before this point are seen by all lanes after it
//   BI_STATES                  lane states the caller holds: 1 on the device (the lane's own), 64 on the host
//   BI_EACH(lane, lane0)       runs the statement after it for every lane the caller stands for
//   BI_I(lane)                 index of that lane's state
// A lane state (BiLane) is uniform over the wave: every lane reads the same bits and takes the same branches.  What differs per
// lane is its share of the work done together: 16 bytes of a half of the ring, the bytes k = lane, lane + 64, ... of a match or a
// stored block, the symbols s = lane, lane + 64, ... of a Huffman table, 16 bytes of the finished window.
//
// Acceptance follows the host decoder (csrc/inflate.cpp) and is never wider: a Huffman code is taken when it is complete, or one
// single 1-bit code, or no code at all (then every look-up fails); HLIT > 286, HDIST > 30, a repeat without a predecessor or past
// HLIT + HDIST, no code for symbol 256, symbols 286 / 287 and distance symbols 30 / 31 refuse the member.

#ifndef BI_FN
#error "define BI_FN, BI_LD_IN16, BI_LD_IN8, BI_ST_OUT16, BI_ST_OUT8, BI_ATOMIC_INC, BI_SYNC, BI_STATES, BI_EACH and BI_I first"
#endif

#define BI_LANES 64
#define BI_WINDOW 65536                  // the member's whole text
#define BI_RING 2048                     // staged compressed bytes: two halves
#define BI_HALF 1024
#define BI_RING_WORDS (BI_RING / 4)

// why a member was not taken (MPB_BGZF_WHY_* of include/moira_pb.h, checked equal in the kernel unit)
#define BI_OK 0
#define BI_HEADER 1
#define BI_BTYPE 2
#define BI_STORED 3
#define BI_CLCODE 4
#define BI_REPEAT 5
#define BI_TREE 6
#define BI_SYMBOL 7
#define BI_DISTANCE 8
#define BI_OVERRUN 9
#define BI_SHORT 10
#define BI_TRUNCATED 11
#define BI_TRAILING 12
#define BI_CRC 13

// One canonical Huffman code: codes of at most FB bits are looked up in `fast` (entry = symbol << 4 | length, 0 = none), longer
// ones -- and the decision "no such code" -- by walking the lengths over count / sorted, one bit per step.
template <int FB, int NS> struct BiTree {
    uint16_t fast[1 << FB];
    uint16_t sorted[NS];                 // symbols in order of (length, symbol)
    uint16_t first[16], offs[16];        // per length: its first code, and where its symbols start in sorted
    uint32_t count[16];                  // symbols per length (count[0] unused)
};
typedef BiTree<10, 288> BiLitTree;
typedef BiTree<8, 32> BiDistTree;
typedef BiTree<7, 20> BiClTree;

struct BiShared {                        // the wave's shared memory beside the window
    uint32_t ring[BI_RING_WORDS];
    BiLitTree dyn_lit, fix_lit;
    BiDistTree dyn_dist, fix_dist;
    BiClTree cl;
    uint8_t lens[320];                   // code lengths of the block being set up: HLIT, then HDIST
    uint8_t cl_lens[20];
};

enum { BI_EV_LIT = 0, BI_EV_MATCH = 1, BI_EV_EOB = 2, BI_EV_ERR = 3 };

struct BiLane {
    uint64_t bb;                         // bit buffer: the next bits of the stream, least significant first
    uint32_t bitcnt;                     // valid bits in bb
    uint32_t widx;                       // next 32-bit word to load; byte 4 * widx counted from the aligned start below the stream
    uint32_t fill_base;                  // the ring holds the bytes [fill_base, fill_base + BI_RING), same origin
    uint32_t used, total_bits;           // bits consumed of the stream, and 8 * stream_len
    uint32_t out, out_len;               // text bytes produced, and ISIZE
    uint32_t why, ev;
    uint32_t bfinal, btype, stored_len, hlit, hdist, fixed_ready;
    uint32_t stored_blocks, fixed_blocks, dynamic_blocks, literals, matches, matched_bytes, longest_code;
};

// ---- bit reader ------------------------------------------------------------------------------------------------------------------
BI_FN void bi_refill(BiLane *L, const uint32_t *ring)       // at least 32 valid bits afterwards
{
    if (L->bitcnt <= 32) {
        L->bb |= (uint64_t)ring[L->widx & (BI_RING_WORDS - 1)] << L->bitcnt;
        L->bitcnt += 32;
        L->widx++;
    }
}
BI_FN uint32_t bi_peek(const BiLane *L, uint32_t n) { return (uint32_t)L->bb & ((1u << n) - 1u); }     // n < 32
BI_FN void bi_drop(BiLane *L, uint32_t n) { L->bb >>= n; L->bitcnt -= n; L->used += n; }
BI_FN bool bi_past_end(BiLane *L)
{
    if (L->used <= L->total_bits) return false;
    L->why = BI_TRUNCATED;
    return true;
}

BI_FN bool bi_near_end(const BiLane *L) { return L->used + 15u > L->total_bits; }    // the look-up saw bits past the end

// the reader at byte `at` (same origin as widx) with `used` bits of the stream behind it; the caller stages both halves next
BI_FN void bi_seek(BiLane *L, uint32_t at, uint32_t used)
{
    L->fill_base = at & ~(uint32_t)(BI_HALF - 1);
    L->bb = 0; L->bitcnt = 0; L->widx = at >> 2; L->used = used;
}
BI_FN void bi_seek_finish(BiLane *L, const uint32_t *ring, uint32_t at)
{
    bi_refill(L, ring);
    const uint32_t skip = 8u * (at & 3u);
    L->bb >>= skip; L->bitcnt -= skip;
}

// This lane's 16 bytes of the half [base, base + BI_HALF) of the ring.  a0 is the origin as an offset into `in` (a multiple of 16),
// [lo, hi) the stream's bytes as offsets into `in`: nothing outside them is loaded, and what lies outside reads as zero.
BI_FN void bi_stage_half(uint32_t *ring, const uint8_t *in, int64_t a0, uint32_t base, int64_t lo, int64_t hi, int lane)
{
    const uint32_t rel = base + 16u * (uint32_t)lane;
    const int64_t q = a0 + (int64_t)rel;
    uint32_t w[4] = {0, 0, 0, 0};
    if (q >= lo && q + 16 <= hi) {
        BI_LD_IN16(in, q, w);
    } else if (q + 16 > lo && q < hi) {
        for (int k = 0; k < 16; k++) {
            const int64_t p = q + k;
            if (p >= lo && p < hi) w[k >> 2] |= (uint32_t)BI_LD_IN8(in, p) << (8 * (k & 3));
        }
    }
    uint32_t *dst = ring + ((rel & (uint32_t)(BI_RING - 1)) >> 2);
    dst[0] = w[0]; dst[1] = w[1]; dst[2] = w[2]; dst[3] = w[3];
}

// ---- Huffman tables, built by the lanes together: clear, count, plan (uniform), place -----------------------------------------
BI_FN uint32_t bi_reverse(uint32_t v, int n)                // the low n bits of v (n <= 15) in reverse order
{
    v = ((v & 0x5555u) << 1) | ((v >> 1) & 0x5555u);
    v = ((v & 0x3333u) << 2) | ((v >> 2) & 0x3333u);
    v = ((v & 0x0f0fu) << 4) | ((v >> 4) & 0x0f0fu);
    v = ((v & 0x00ffu) << 8) | ((v >> 8) & 0x00ffu);
    return v >> (16 - n);
}

template <int FB, int NS> BI_FN void bi_tree_clear(BiTree<FB, NS> *t, int lane)
{
    for (int i = lane; i < (1 << FB); i += BI_LANES) t->fast[i] = 0;
    if (lane < 16) t->count[lane] = 0;
}

template <int FB, int NS> BI_FN void bi_tree_count(BiTree<FB, NS> *t, const uint8_t *lens, int n, int lane)
{
    for (int s = lane; s < n && s < NS; s += BI_LANES) {
        const uint32_t l = lens[s];
        if (l >= 1 && l <= 15) BI_ATOMIC_INC(&t->count[l]);
    }
}

// uniform: every lane writes the same first / offs.  false: the code is over-subscribed or incomplete (inflate.cpp's build_table)
template <int FB, int NS> BI_FN bool bi_tree_plan(BiTree<FB, NS> *t, BiLane *L)
{
    int used = 0, left = 1;
    uint32_t code = 0, idx = 0, longest = 0;
    bool over = false;
    for (int l = 1; l <= 15; l++) {
        const uint32_t c = t->count[l];
        used += (int)c;
        left = left * 2 - (int)c;
        if (left < 0) { over = true; left = 0; }
        t->first[l] = (uint16_t)code;
        t->offs[l] = (uint16_t)idx;
        code = (code + c) << 1;
        idx += c;
        if (c) longest = (uint32_t)l;
    }
    if (used == 0) return true;                              // no code at all: every look-up fails
    if (over) return false;
    if (left > 0 && !(used == 1 && t->count[1] == 1)) return false;
    if (longest > L->longest_code) L->longest_code = longest;
    return true;
}

template <int FB, int NS> BI_FN void bi_tree_place(BiTree<FB, NS> *t, const uint8_t *lens, int n, int lane)
{
    for (int s = lane; s < n && s < NS; s += BI_LANES) {
        const uint32_t l = lens[s];
        if (l < 1 || l > 15) continue;
        uint32_t rank = 0;
        for (int j = 0; j < s; j++) rank += lens[j] == l ? 1u : 0u;
        const uint32_t at = (uint32_t)t->offs[l] + rank;
        if (at < (uint32_t)NS) t->sorted[at] = (uint16_t)s;
        if (l <= (uint32_t)FB) {
            const uint32_t r = bi_reverse(((uint32_t)t->first[l] + rank) & 0x7fffu, (int)l);
            const uint16_t e = (uint16_t)(((uint32_t)s << 4) | l);
            for (uint32_t k = r; k < (1u << FB); k += 1u << l) t->fast[k] = e;
        }
    }
}

// symbol << 4 | code length for the code at the low end of `bits` (15 bits of the stream), 0: no such code
template <int FB, int NS> BI_FN uint32_t bi_decode(const BiTree<FB, NS> *t, uint32_t bits)
{
    const uint32_t e = t->fast[bits & ((1u << FB) - 1u)];
    if (e) return e;
    uint32_t code = 0, first = 0, index = 0;
    for (uint32_t len = 1; len <= 15; len++) {
        code |= (bits >> (len - 1)) & 1u;
        const uint32_t cnt = t->count[len];
        if (code >= first && code - first < cnt) {
            const uint32_t at = index + (code - first);
            return at < (uint32_t)NS ? ((uint32_t)t->sorted[at] << 4) | len : 0u;
        }
        index += cnt;
        first = (first + cnt) << 1;
        code <<= 1;
    }
    return 0;
}

// ---- block header (uniform) ------------------------------------------------------------------------------------------------------
BI_FN void bi_block_header(BiLane *L, BiShared *sh, uint32_t stream_len)
{
    static const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    bi_refill(L, sh->ring);
    L->bfinal = bi_peek(L, 1); bi_drop(L, 1);
    L->btype = bi_peek(L, 2); bi_drop(L, 2);
    if (bi_past_end(L)) return;
    if (L->btype == 3) { L->why = BI_BTYPE; return; }
    if (L->btype == 0) {
        bi_drop(L, (8u - (L->used & 7u)) & 7u);
        bi_refill(L, sh->ring);
        const uint32_t len = bi_peek(L, 16); bi_drop(L, 16);
        const uint32_t nlen = bi_peek(L, 16); bi_drop(L, 16);
        if (bi_past_end(L)) return;
        if ((len ^ nlen) != 0xffffu) { L->why = BI_STORED; return; }
        if (L->out + len > L->out_len) { L->why = BI_OVERRUN; return; }
        if ((L->used >> 3) + len > stream_len) { L->why = BI_TRUNCATED; return; }
        L->stored_len = len;
        L->stored_blocks++;
        return;
    }
    if (L->btype == 1) { L->fixed_blocks++; return; }
    bi_refill(L, sh->ring);
    L->hlit = bi_peek(L, 5) + 257u; bi_drop(L, 5);
    L->hdist = bi_peek(L, 5) + 1u; bi_drop(L, 5);
    const uint32_t hclen = bi_peek(L, 4) + 4u; bi_drop(L, 4);
    if (bi_past_end(L)) return;
    if (L->hlit > 286u || L->hdist > 30u) { L->why = BI_TREE; return; }
    for (int i = 0; i < 20; i++) sh->cl_lens[i] = 0;
    for (uint32_t i = 0; i < hclen; i++) {
        bi_refill(L, sh->ring);
        sh->cl_lens[order[i]] = (uint8_t)bi_peek(L, 3); bi_drop(L, 3);
    }
    if (bi_past_end(L)) return;
    L->dynamic_blocks++;
}

// the HLIT + HDIST code lengths of a dynamic block through the code-length code (uniform; at most 320 * 14 bits)
BI_FN void bi_read_lengths(BiLane *L, BiShared *sh)
{
    const uint32_t total = L->hlit + L->hdist;
    uint32_t k = 0;
    while (k < total) {
        bi_refill(L, sh->ring);
        const uint32_t e = bi_decode(&sh->cl, (uint32_t)L->bb & 0x7fffu);
        if (!e) { L->why = bi_near_end(L) ? BI_TRUNCATED : BI_CLCODE; return; }
        bi_drop(L, e & 15u);
        const uint32_t sym = e >> 4;
        if (sym < 16u) {
            if (bi_past_end(L)) return;
            sh->lens[k++] = (uint8_t)sym;
            continue;
        }
        uint32_t rep, val = 0;
        if (sym == 16u) {
            if (k == 0) { L->why = bi_past_end(L) ? BI_TRUNCATED : BI_REPEAT; return; }
            val = sh->lens[k - 1];
            rep = 3u + bi_peek(L, 2); bi_drop(L, 2);
        } else if (sym == 17u) {
            rep = 3u + bi_peek(L, 3); bi_drop(L, 3);
        } else if (sym == 18u) {
            rep = 11u + bi_peek(L, 7); bi_drop(L, 7);
        } else { L->why = BI_CLCODE; return; }
        if (bi_past_end(L)) return;
        if (k + rep > total) { L->why = BI_REPEAT; return; }
        while (rep--) sh->lens[k++] = (uint8_t)val;
    }
    if (sh->lens[256] == 0) L->why = BI_TREE;                // no end-of-block code
}

// the fixed code's lengths: 288 literal / length symbols, then 32 distance symbols
BI_FN void bi_fixed_lens(uint8_t *lens, int lane)
{
    for (int s = lane; s < 320; s += BI_LANES) lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < 288 ? 8 : 5);
}

// ---- one symbol: decode (uniform) and this lane's share of what it writes ----------------------------------------------------------
// A literal is stored by lane 0.  A match of `len` at distance `d` copies byte k from out - d + (k mod d): when d >= len that is the
// plain copy, 64 bytes per step; when d < len it is the byte-serial result (every source byte lies before `out`, so no lane reads
// what another writes in the same match).
BI_FN void bi_symbol(BiLane *L, const uint32_t *ring, const BiLitTree *lit, const BiDistTree *dist, uint8_t *window, int lane)
{
    L->ev = BI_EV_ERR;
    bi_refill(L, ring);
    uint32_t e = bi_decode(lit, (uint32_t)L->bb & 0x7fffu);
    if (!e) { L->why = bi_near_end(L) ? BI_TRUNCATED : BI_SYMBOL; return; }
    bi_drop(L, e & 15u);
    const uint32_t sym = e >> 4;
    if (sym < 256u) {
        if (bi_past_end(L)) return;
        if (L->out >= L->out_len) { L->why = BI_OVERRUN; return; }
        if (lane == 0) window[L->out] = (uint8_t)sym;
        L->out++; L->literals++;
        L->ev = BI_EV_LIT;
        return;
    }
    if (sym == 256u) {
        if (bi_past_end(L)) return;
        L->ev = BI_EV_EOB;
        return;
    }
    if (sym > 285u) { L->why = bi_past_end(L) ? BI_TRUNCATED : BI_SYMBOL; return; }
    const uint32_t i = sym - 257u;
    uint32_t len;
    if (i < 8u) len = 3u + i;
    else if (i == 28u) len = 258u;
    else {
        const uint32_t x = (i - 4u) >> 2;
        len = 3u + ((4u + (i & 3u)) << x) + bi_peek(L, x);
        bi_drop(L, x);
    }
    bi_refill(L, ring);
    e = bi_decode(dist, (uint32_t)L->bb & 0x7fffu);
    if (!e) { L->why = bi_near_end(L) ? BI_TRUNCATED : BI_DISTANCE; return; }
    bi_drop(L, e & 15u);
    const uint32_t ds = e >> 4;
    if (ds > 29u) { L->why = bi_past_end(L) ? BI_TRUNCATED : BI_DISTANCE; return; }
    uint32_t d;
    if (ds < 4u) d = ds + 1u;
    else {
        const uint32_t x = (ds >> 1) - 1u;
        d = 1u + ((2u + (ds & 1u)) << x) + bi_peek(L, x);
        bi_drop(L, x);
    }
    if (bi_past_end(L)) return;
    if (d > L->out) { L->why = BI_DISTANCE; return; }
    if (L->out + len > L->out_len) { L->why = BI_OVERRUN; return; }
    const uint32_t from = L->out - d;
    for (uint32_t k = (uint32_t)lane; k < len; k += BI_LANES) window[L->out + k] = window[from + (d >= len ? k : k % d)];
    L->out += len; L->matches++; L->matched_bytes += len;
    L->ev = BI_EV_MATCH;
}

// ---- the finished window -> text + out_off: bytes up to the first 16-byte boundary of the text, 16 bytes per lane, bytes again ----
BI_FN uint32_t bi_window_word(const uint32_t *window32, uint32_t at)       // the four bytes at window + at, any alignment
{
    const uint32_t w = at >> 2, sh = 8u * (at & 3u);
    const uint32_t lo = window32[w];
    if (!sh) return lo;
    const uint32_t hi = w + 1u < (uint32_t)(BI_WINDOW / 4) ? window32[w + 1u] : 0u;
    return (lo >> sh) | (hi << (32u - sh));
}

BI_FN void bi_store_window(const uint32_t *window32, uint8_t *text, int64_t out_off, uint32_t out_len, int lane)
{
    const uint8_t *window = (const uint8_t *)window32;
    uint32_t head = (16u - (uint32_t)(out_off & 15)) & 15u;
    if (head > out_len) head = out_len;
    for (uint32_t k = (uint32_t)lane; k < head; k += BI_LANES) BI_ST_OUT8(text, out_off + (int64_t)k, window[k]);
    const uint32_t nvec = (out_len - head) >> 4;
    for (uint32_t v = (uint32_t)lane; v < nvec; v += BI_LANES) {
        const uint32_t at = head + 16u * v;
        uint32_t w[4];
        for (uint32_t j = 0; j < 4; j++) w[j] = bi_window_word(window32, at + 4u * j);
        BI_ST_OUT16(text, out_off + (int64_t)at, w);
    }
    for (uint32_t k = head + 16u * nvec + (uint32_t)lane; k < out_len; k += BI_LANES) BI_ST_OUT8(text, out_off + (int64_t)k, window[k]);
}

// ---- one member, by the wave (device: BI_EACH runs its statement once, for this lane; host: for all 64 in turn) -------------------
// in[in_bytes]: the piece's compressed bytes; the stream is in[stream_off, stream_off + stream_len), already checked to lie inside
// with stream_len <= 65536, and out_len <= BI_WINDOW.  Returns the member's status (BI_OK: window[0, out_len) is its text).
#define BI_ALL(...) BI_EACH(lane, lane0) { BiLane *Lp = &L[BI_I(lane)]; (void)Lp; (void)lane; __VA_ARGS__; }
#define BI_BUILD(tree, lens_ptr, n_syms, why_code)                                                  \
    do {                                                                                            \
        BI_ALL(bi_tree_clear((tree), lane)) BI_SYNC();                                              \
        BI_ALL(bi_tree_count((tree), (lens_ptr), (int)(n_syms), lane)) BI_SYNC();                   \
        BI_ALL(if (!bi_tree_plan((tree), Lp)) Lp->why = (why_code)) BI_SYNC();                      \
        if (!L[0].why) { BI_ALL(bi_tree_place((tree), (lens_ptr), (int)(n_syms), lane)) BI_SYNC(); } \
    } while (0)
#define BI_ADVANCE()                                                                                \
    while ((L[0].widx << 2) >= L[0].fill_base + (uint32_t)BI_HALF) {                                \
        BI_ALL(bi_stage_half(sh->ring, in, a0, Lp->fill_base + (uint32_t)BI_RING, lo, hi, lane);    \
               Lp->fill_base += (uint32_t)BI_HALF)                                                  \
        BI_SYNC();                                                                                  \
    }
#define BI_SEEK(at_expr, used_expr)                                                                 \
    do {                                                                                            \
        BI_ALL(bi_seek(Lp, (at_expr), (used_expr));                                                 \
               bi_stage_half(sh->ring, in, a0, Lp->fill_base, lo, hi, lane);                        \
               bi_stage_half(sh->ring, in, a0, Lp->fill_base + (uint32_t)BI_HALF, lo, hi, lane))    \
        BI_SYNC();                                                                                  \
        BI_ALL(bi_seek_finish(Lp, sh->ring, (at_expr)))                                             \
    } while (0)

BI_FN uint32_t bi_member(const uint8_t *in, int64_t stream_off, uint32_t stream_len, uint32_t out_len, uint8_t *window,
                         BiShared *sh, BiLane *L, int lane0, uint32_t *iterations)
{
    const int64_t a0 = stream_off & ~(int64_t)15, lo = stream_off, hi = stream_off + (int64_t)stream_len;
    const uint32_t head = (uint32_t)(stream_off - a0);
    const uint32_t max_iter = 8u * stream_len + 8u;
    uint32_t iter = 0;
    BI_ALL(BiLane z = {}; *Lp = z; Lp->total_bits = 8u * stream_len; Lp->out_len = out_len)
    BI_SEEK(head, 0u);
    for (;;) {
        if (++iter > max_iter) { BI_ALL(Lp->why = BI_TRUNCATED) break; }
        BI_ADVANCE()
        BI_ALL(bi_block_header(Lp, sh, stream_len)) BI_SYNC();
        if (L[0].why) break;
        if (L[0].btype == 0) {
            // a stored block: all lanes copy stream bytes into the window; the reader starts again behind it
            BI_ALL(const uint32_t src = Lp->used >> 3;
                   for (uint32_t k = (uint32_t)lane; k < Lp->stored_len; k += BI_LANES)
                       window[Lp->out + k] = BI_LD_IN8(in, lo + (int64_t)(src + k));
                   Lp->out += Lp->stored_len; Lp->used += 8u * Lp->stored_len)
            BI_SYNC();
            BI_SEEK(head + (Lp->used >> 3), Lp->used);
        } else {
            const BiLitTree *lit;
            const BiDistTree *dist;
            if (L[0].btype == 2) {
                BI_BUILD(&sh->cl, sh->cl_lens, 19, BI_CLCODE);
                if (L[0].why) break;
                BI_ADVANCE()
                BI_ALL(bi_read_lengths(Lp, sh)) BI_SYNC();
                if (L[0].why) break;
                BI_BUILD(&sh->dyn_lit, sh->lens, L[0].hlit, BI_TREE);
                if (L[0].why) break;
                BI_BUILD(&sh->dyn_dist, sh->lens + L[0].hlit, L[0].hdist, BI_TREE);
                if (L[0].why) break;
                lit = &sh->dyn_lit; dist = &sh->dyn_dist;
            } else {
                if (!L[0].fixed_ready) {
                    BI_ALL(bi_fixed_lens(sh->lens, lane)) BI_SYNC();
                    BI_BUILD(&sh->fix_lit, sh->lens, 288, BI_TREE);
                    BI_BUILD(&sh->fix_dist, sh->lens + 288, 32, BI_TREE);
                    if (L[0].why) break;
                    BI_ALL(Lp->fixed_ready = 1u)
                }
                lit = &sh->fix_lit; dist = &sh->fix_dist;
            }
            for (;;) {                                       // every symbol consumes at least one bit or ends the block
                if (++iter > max_iter) { BI_ALL(Lp->why = BI_TRUNCATED) break; }
                BI_ADVANCE()
                BI_ALL(bi_symbol(Lp, sh->ring, lit, dist, window, lane)) BI_SYNC();
                if (L[0].ev >= BI_EV_EOB) break;
            }
            if (L[0].why) break;
        }
        if (L[0].bfinal) break;
    }
    if (!L[0].why) {
        // the final block ended: the text must be whole and the stream used up to its last byte
        if (L[0].out != out_len) { BI_ALL(Lp->why = BI_SHORT) }
        else if (((L[0].used + 7u) >> 3) != stream_len) { BI_ALL(Lp->why = BI_TRAILING) }
    }
    *iterations = iter;
    return L[0].why;
}
