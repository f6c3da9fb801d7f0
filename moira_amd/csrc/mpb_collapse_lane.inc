// mpb_collapse_lane.inc -- what ONE LANE of the collapse kernels does (mpb_collapse_kernels.hip: k_col_hash, k_col_group,
// k_col_rep), with no wave intrinsic in it: one lane owns one record, so that a host program runs the same text with checked
// loads and stores and modelled atomics (tests/helpers/collapse_lane_check.cpp).  The step stands between a text with its record
// index and mio_collapse_add_grouped (csrc/fastio.cpp): for every record the CPython-2.7 string hash of its (truncated) sequence
// -- py2_hash there is the yardstick -- and the first record of the chunk with the same sequence.
// The includer defines
//     CL_FN                         the function qualifier (__device__ __forceinline__ / static inline)
//     CL_LD_I64(p, k)               p[k] of the index, asked for only inside its rows
//     CL_LD_U64(p, k)               hash[k], k < n: written before the launch that reads it (k_col_hash's, read by k_col_group)
//     CL_LD_U32(p, k)               first[s], s < cap, read by k_col_rep only (after k_col_group's launch has ended)
//     CL_LD_SLOT(p, k)              slot[k], k < n, likewise
//     CL_LD16(text, off)            the aligned 16 bytes at text + off (off % 16 == 0) as a cl_w16, asked for only when a byte of
//                                   a validated range lies in them: below round_up(text_bytes, 16)
//     CL_ST_U64(p, k, v)            hash[k] = v;  CL_ST_I32(p, k, v): rep[k] = v;  CL_ST_SLOT(p, k, v): slot[k] = v
//     CL_CAS_I32(p, s, want, v)     atomic: if table[s] == want it becomes v; -> what it held
//     CL_MIN_U32(p, s, v)           atomic: first[s] = min(first[s], v)
// Inside k_col_group the lanes talk to each other through the RETURN VALUES of these two atomics only; every other byte a lane
// reads there (text, index, hash[]) was written before the launch.  Every loop runs over a checked length or over cap.

#define CL_LANES 256                              // lanes of a workgroup: one record each
#define CL_EMPTY (-1)                             // an owner slot nobody has taken
#define CL_NO_SLOT (-1ll)                         // slot[k] of a record that settled nowhere (a failed row; never else)

struct cl_w16 { uint32_t w[4]; };

struct ClParams { int64_t n_records, text_bytes, cap; int32_t max_len, cap_shift; };     // cap = 1 << (64 - cap_shift) >= 2 n

struct ClRow { int64_t seq_off; int32_t L; };     // a record's sequence after every check: the range lies inside the text

// Row k of the index by every check (it is not trusted, uploaded or device-written).  false: nothing of it may be read.
CL_FN bool cl_row(const int64_t *idx, int64_t k, const ClParams &p, ClRow *o)
{
    const int64_t so = CL_LD_I64(idx, k * 6 + 2), sl = CL_LD_I64(idx, k * 6 + 3);
    const bool ok = so >= 0 && sl >= 0 && sl <= 0x7fffffffll && sl <= p.text_bytes && so <= p.text_bytes - sl;
    o->seq_off = ok ? so : 0;
#ifdef CL_NO_MAX_LEN_CLAMP                        // (the checker's sensitivity build: -t / --truncate forgotten)
    o->L = ok ? (int32_t)sl : 0;
#else
    o->L = ok ? (int32_t)(p.max_len > 0 && sl > p.max_len ? p.max_len : sl) : 0;
#endif
    return ok;
}

CL_FN uint32_t cl_byte(const cl_w16 &v, int t) { return (v.w[t >> 2] >> (8 * (t & 3))) & 255u; }

// ---- k_col_hash -------------------------------------------------------------------------------------------------------------
// CPython 2.7's string_hash of text[seq_off, seq_off + L): x = s[0] << 7; x = 1000003 x ^ s[i] for every i; x ^= L; -1 -> -2; 0 for
// an empty string.  One dependent multiply-xor per byte: the chain is this lane's alone.  The aligned words that hold a byte of
// the range are fetched once each (the last one ends below round_up(text_bytes, 16) because a byte of the range lies in it).
CL_FN uint64_t cl_hash(const uint8_t *text, const ClRow &r)
{
    if (r.L <= 0) return 0;
    const int64_t lo = r.seq_off, hi = r.seq_off + r.L;
    uint64_t x = 0;
    for (int64_t w = lo & ~(int64_t)15; w < hi; w += 16) {
        const cl_w16 v = CL_LD16(text, w);
        if (w > lo && w + 16 <= hi) {             // a whole word behind the first byte: nothing to ask per byte
#pragma unroll
            for (int t = 0; t < 16; t++) x = (1000003ull * x) ^ (uint64_t)cl_byte(v, t);
            continue;
        }
#pragma unroll
        for (int t = 0; t < 16; t++) {
            const uint64_t b = cl_byte(v, t);
            if (w + t == lo) x = b << 7;
            if (w + t >= lo && w + t < hi) x = (1000003ull * x) ^ b;
        }
    }
    x ^= (uint64_t)r.L;
    return x == ~0ull ? ~0ull - 1 : x;
}

// ---- k_col_group ------------------------------------------------------------------------------------------------------------
// bytes [sh, sh + 16) of the 32 bytes a | b, sh = 0..15 (k_pack_text's funnel in plain C, as mpb_format_lane.inc has it)
CL_FN cl_w16 cl_funnel16(const cl_w16 &a, const cl_w16 &b, uint32_t sh)
{
    uint32_t w0 = a.w[0], w1 = a.w[1], w2 = a.w[2], w3 = a.w[3], w4 = b.w[0], w5 = b.w[1];
    if (sh & 8u) { w0 = a.w[2]; w1 = a.w[3]; w2 = b.w[0]; w3 = b.w[1]; w4 = b.w[2]; w5 = b.w[3]; }
    if (sh & 4u) { w0 = w1; w1 = w2; w2 = w3; w3 = w4; w4 = w5; }
    const uint32_t bs = 8u * (sh & 3u);
    cl_w16 o;
    o.w[0] = (uint32_t)((((uint64_t)w1 << 32) | w0) >> bs);
    o.w[1] = (uint32_t)((((uint64_t)w2 << 32) | w1) >> bs);
    o.w[2] = (uint32_t)((((uint64_t)w3 << 32) | w2) >> bs);
    o.w[3] = (uint32_t)((((uint64_t)w4 << 32) | w3) >> bs);
    return o;
}

// the 16 bytes at text[s ..), of which the first m (1..16) lie in a validated range: the aligned word of s, and the next one only
// when one of the m bytes lies in it
CL_FN cl_w16 cl_fetch16(const uint8_t *text, int64_t s, int m)
{
    const int64_t base = s & ~(int64_t)15;
    const uint32_t sh = (uint32_t)(s & 15);
    const cl_w16 a = CL_LD16(text, base);
    cl_w16 b;
    b.w[0] = 0; b.w[1] = 0; b.w[2] = 0; b.w[3] = 0;
    if (sh + (uint32_t)m > 16u) b = CL_LD16(text, base + 16);
    return cl_funnel16(a, b, sh);
}

// text[a, a + L) == text[b, b + L), both validated ranges; 16 bytes a step, the bytes behind L masked away
CL_FN bool cl_equal(const uint8_t *text, int64_t a, int64_t b, int32_t L)
{
#ifdef CL_SKIP_BYTE_COMPARE                       // (the checker's sensitivity build: equal hash and length taken for equal bytes)
    (void)text; (void)a; (void)b; (void)L;
    return true;
#else
    if (a == b) return true;
    for (int64_t c = 0; c < L; c += 16) {
        const int m = L - c < 16 ? (int)(L - c) : 16;
        const cl_w16 x = cl_fetch16(text, a + c, m), y = cl_fetch16(text, b + c, m);
        uint32_t diff = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int live = m - 4 * i;           // bytes of word i inside the range
            const uint32_t mask = live >= 4 ? 0xffffffffu : live <= 0 ? 0u : (1u << (8 * live)) - 1u;
            diff |= (x.w[i] ^ y.w[i]) & mask;
        }
        if (diff) return false;
    }
    return true;
#endif
}

// where a hash starts to probe (the low bits of a string hash are its last byte's: the host's shard tables multiply as well)
CL_FN int64_t cl_start(uint64_t h, const ClParams &p) { return (int64_t)((h * 0x9E3779B97F4A7C15ull) >> p.cap_shift); }

// Record k settles on the owner slot of its sequence: linear probing from cl_start, ONE compare-and-swap of empty -> k per slot.
// It owns the slot if it wins; it stays on owner j's slot iff hash, length and bytes agree; else the next slot.  All records of
// one sequence start at one slot and pass a slot only when its (final, never changing) owner differs from them, so they settle
// on the same slot whoever owns it; first[slot] = the smallest of them is then independent of scheduling.  No lane waits for
// another: cap >= 2 n owners' slots can not fill, and the walk ends after cap slots whatever the table holds.
// The walk is cut into its steps (one atomic each) so that the host model can run the lanes in lockstep.
struct ClProbe { ClRow r; uint64_t h; int64_t s, left, at; };     // at: the slot settled on, CL_NO_SLOT while walking (or for ever)

CL_FN void cl_probe_begin(const int64_t *idx, const uint64_t *hash, int64_t k, const ClParams &p, ClProbe *w)
{
    w->h = 0; w->s = 0; w->left = 0; w->at = CL_NO_SLOT;
    if (!cl_row(idx, k, p, &w->r)) return;         // (k_col_hash said so already: no walk)
    w->h = CL_LD_U64(hash, k);
    w->s = cl_start(w->h, p);
    w->left = p.cap;
}

// one slot of the walk; -> false when the walk is over
CL_FN bool cl_probe_step(const uint8_t *text, const int64_t *idx, const uint64_t *hash, int64_t k, const ClParams &p, int32_t *table,
                         ClProbe *w)
{
    if (w->left <= 0 || w->at != CL_NO_SLOT) return false;
    const int32_t seen = CL_CAS_I32(table, w->s, CL_EMPTY, (int32_t)k);
    const int64_t j = seen == CL_EMPTY ? k : (int64_t)seen;
    bool mine = j == k;
    if (!mine && j >= 0 && j < p.n_records && CL_LD_U64(hash, j) == w->h) {
        ClRow o;
        mine = cl_row(idx, j, p, &o) && o.L == w->r.L && cl_equal(text, w->r.seq_off, o.seq_off, w->r.L);
    }
    if (mine) { w->at = w->s; return false; }
    w->s = (w->s + 1) & (p.cap - 1);
    w->left--;
    return w->left > 0;
}

CL_FN void cl_probe_end(int64_t k, const ClProbe &w, uint32_t *first, int64_t *slot)
{
    if (w.at != CL_NO_SLOT) CL_MIN_U32(first, w.at, (uint32_t)k);
    CL_ST_SLOT(slot, k, w.at);
}

// ---- k_col_rep --------------------------------------------------------------------------------------------------------------
// rep[k] = the smallest record on k's slot: the smallest k' <= k with an equal sequence (k itself for a record without a slot)
CL_FN void cl_rep(const uint32_t *first, const int64_t *slot, int64_t k, int32_t *rep)
{
    const int64_t s = CL_LD_SLOT(slot, k);
    CL_ST_I32(rep, k, s == CL_NO_SLOT ? (int32_t)k : (int32_t)CL_LD_U32(first, s));
}
