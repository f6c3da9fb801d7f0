// mpb_fasta_qual_lane.inc -- what ONE LANE of the fasta+qual record stage does (mpb_fasta_qual_kernels.hip: k_fa_count,
// k_fa_write), with no wave intrinsic in it: a neighbour's count is an argument, so that a host program runs the same text with
// checked loads and stores (tests/helpers/fasta_qual_lane_check.cpp).  The stage stands behind the line kernels of the FASTQ
// index (k_fq_lines / k_fq_scan / k_fq_starts, run over both texts): record r is lines 2 r and 2 r + 1 of the fasta text and of
// the qual text, and becomes one slot `header token | sequence | one byte per quality` of the buffer mio_fasta_qual_index builds.
// The rules are mio_fasta_qual_index's (csrc/fastio.cpp); that function is the yardstick and the only code that defines an
// error.  The lanes refuse a superset of what it refuses: a quality token takes one to three digits here (the host also reads
// "0007"), and every candidate record is looked at, also behind the first that does not fit the caller's buffer.
// The includer defines, before this file,
//     FA_FN                        the function qualifier (__device__ __forceinline__ / static inline)
//     FQ_FN, FqWord, FQ_LDW, FQ_LDB, FQ_LD_START, FQ_ST_START     as mpb_index_lane.inc asks for them (it is included here);
//                                  a load names its text, so an includer with checked loads tells the two texts apart by that
//     FA_ST8(o, pos, byte)         out[pos] = byte; o is the includer's, and knows the record's own slot
// Every loop here runs over the 16 bytes of a word (and the four before it), the blanks of a line's ends or a header line.

#include "mpb_index_lane.inc"

#define FA_LANES 256                              // lanes of a workgroup of k_fa_count / k_fa_write
#define FA_GROUP 8                                // lanes that share one record, as in k_fmt_count
#define FA_STRIDE (FA_GROUP * FQ_WORD_BYTES)      // quality text a group takes per step
// why a record is not taken (MPB_FQ_WHY_ROW_CHECK and MPB_FA_WHY_* of include/moira_pb.h, restated)
#define FA_WHY_ROW_CHECK 4
#define FA_WHY_NAMES     5
#define FA_WHY_EMPTY     6
#define FA_WHY_TOKEN     7
#define FA_WHY_LENGTH    8

// a record's spans: header token and sequence in the fasta text, header token and quality line in the qual text
struct FaRec { int64_t hdr_off, hdr_len, seq_off, seq_len, qhdr_off, qhdr_len, q_off, q_len; };

// what the status word holds for the first record that is not taken: the smallest key wins (atomic min)
FA_FN long long fa_key(int64_t r, int why, int which) { return (long long)((r << 8) | (int64_t)(why << 1) | (int64_t)which); }

// Lines 2 r and 2 r + 1 of a text, stripped.  start[] is device-written and not trusted: false, with nothing read of the text,
// unless 0 <= start < next start <= text_bytes for both lines (fq_row's check).
FA_FN bool fa_lines(const uint8_t *text, int64_t text_bytes, const uint32_t *start, int64_t n_start, int64_t r, int64_t off[2],
                    int64_t len[2])
{
    off[0] = off[1] = 0; len[0] = len[1] = 0;
    if (r < 0 || 2 * r + 2 >= n_start) return false;
    int64_t s[3];
    for (int k = 0; k < 3; k++) s[k] = (int64_t)FQ_LD_START(start, 2 * r + k);
    if (s[0] >= s[1] || s[1] >= s[2] || s[2] > text_bytes) return false;
    for (int k = 0; k < 2; k++) {
        int64_t e = s[k + 1];
        if (FQ_LDB(text, e - 1) == 0x0au) e--;               // (otherwise: the unterminated last line, which ends at the text's end)
        fq_strip(text, s[k], e, &off[k], &len[k]);
    }
    return true;
}

// header: replace('\t', ' ').split(' ')[0].lstrip('>')
FA_FN void fa_token(const uint8_t *text, int64_t off, int64_t len, int64_t *t_off, int64_t *t_len)
{
    int64_t h0 = off, h1 = off;
    const int64_t hend = off + len;
    while (h1 < hend) {
        const uint32_t c = FQ_LDB(text, h1);
        if (c == 0x20u || c == 0x09u) break;
        h1++;
    }
    while (h0 < h1 && FQ_LDB(text, h0) == 0x3eu) h0++;
    *t_off = h0; *t_len = h1 - h0;
}

// The spans of record r.  -> 0, or why the record is not taken for a reason its lines show (*which: the text it speaks of).
// `names`: compare the two header tokens (k_fa_count does; k_fa_write runs behind it).
FA_FN int fa_record(const uint8_t *ftext, int64_t fbytes, const uint32_t *fstart, int64_t n_fstart, const uint8_t *qtext,
                    int64_t qbytes, const uint32_t *qstart, int64_t n_qstart, int64_t r, bool names, FaRec *o, int *which)
{
    int64_t off[2], len[2];
    o->hdr_off = 0; o->hdr_len = 0; o->seq_off = 0; o->seq_len = 0; o->qhdr_off = 0; o->qhdr_len = 0; o->q_off = 0; o->q_len = 0;
    *which = 0;
    if (!fa_lines(ftext, fbytes, fstart, n_fstart, r, off, len)) return FA_WHY_ROW_CHECK;
    fa_token(ftext, off[0], len[0], &o->hdr_off, &o->hdr_len);
    o->seq_off = off[1]; o->seq_len = len[1];
    *which = 1;
    if (!fa_lines(qtext, qbytes, qstart, n_qstart, r, off, len)) return FA_WHY_ROW_CHECK;
    fa_token(qtext, off[0], len[0], &o->qhdr_off, &o->qhdr_len);
    o->q_off = off[1]; o->q_len = len[1];
    if (names) {
        bool same = o->hdr_len == o->qhdr_len;
        for (int64_t i = 0; same && i < o->hdr_len; i++) same = FQ_LDB(ftext, o->hdr_off + i) == FQ_LDB(qtext, o->qhdr_off + i);
        if (!same) return FA_WHY_NAMES;
    }
    if (o->seq_len == 0) { *which = 0; return FA_WHY_EMPTY; }
    if (o->q_len == 0) return FA_WHY_EMPTY;
    return 0;
}

// the record's slot: header token | sequence | one byte per base
FA_FN int64_t fa_slot_bytes(const FaRec &r) { return r.hdr_len + 2 * r.seq_len; }

// the aligned words of the quality line: first, and one behind the last
FA_FN int64_t fa_first_word(const FaRec &r) { return r.q_off >> 4; }
FA_FN int64_t fa_end_word(const FaRec &r) { return ((r.q_off + r.q_len - 1) >> 4) + 1; }

// One aligned word of the quality line with the four bytes before it: bit j of the masks and byte j of b speak of text byte
// 16 w - 4 + j, j = 0..19; bit 20 of term: the line ends with the word's last byte.  A byte outside the line sets no bit.
//   dig  a digit            sep  a blank or a tab            bad  a byte of the WORD (j >= 4) that is neither
//   term what ends a token, seen from the word that holds it: a separator of the word, or the first byte behind the line
// A token's digits lie in the three bytes before its terminator, so the carry between words is what b[0] holds.
struct FaQ { int64_t base; uint32_t b[5], dig, sep, term, bad; };   // base: the text byte bit 0 speaks of

FA_FN void fa_qload(const uint8_t *qtext, const FaRec &r, int64_t w, FaQ *o)
{
    const int64_t base = w * FQ_WORD_BYTES - 4, end = r.q_off + r.q_len;
    const FqWord v = FQ_LDW(qtext, w);
    o->base = base;
    o->b[0] = 0;
    if (base + 4 > r.q_off) o->b[0] = FQ_LDW(qtext, w - 1).w;        // (w - 1 >= the line's first word: inside the text)
    o->b[1] = v.x; o->b[2] = v.y; o->b[3] = v.z; o->b[4] = v.w;
    const int lo = r.q_off - base > 0 ? (int)(r.q_off - base) : 0;
    const int hi = end - base < 20 ? (int)(end - base) : 20;         // (>= 5: the word holds a byte of the line)
    uint32_t dig = 0, sep = 0, oth = 0;
#pragma unroll
    for (int j = 0; j < 20; j++) {
        const uint32_t c = (o->b[j >> 2] >> (8 * (j & 3))) & 0xffu;
        const uint32_t in = (j >= lo && j < hi) ? 1u : 0u;
        const uint32_t d = (c - 0x30u <= 9u) ? 1u : 0u, s = (c == 0x20u || c == 0x09u) ? 1u : 0u;
        dig |= (in & d) << j;
        sep |= (in & s) << j;
        oth |= (in & (1u ^ (d | s))) << j;
    }
    o->dig = dig; o->sep = sep; o->bad = oth & 0xffff0u;
    o->term = sep & 0xffff0u;
    if (end - base <= 20) o->term |= 1u << (int)(end - base);        // (5..20: the line ends in this word or with it)
}

// the value of the token that the terminator at bit t (4..20) ends: its last digit at t - 1, up to two more before it
FA_FN uint32_t fa_value(const FaQ &q, int t)
{
    const uint32_t d1 = ((q.b[(t - 1) >> 2] >> (8 * ((t - 1) & 3))) & 0xffu) - 0x30u;
    const uint32_t d2 = ((q.b[(t - 2) >> 2] >> (8 * ((t - 2) & 3))) & 0xffu) - 0x30u;
    const uint32_t d3 = ((q.b[(t - 3) >> 2] >> (8 * ((t - 3) & 3))) & 0xffu) - 0x30u;
    const uint32_t has2 = (q.dig >> (t - 2)) & 1u, has3 = has2 & ((q.dig >> (t - 3)) & 1u);
    return d1 + has2 * 10u * d2 + has3 * 100u * d3;
}

// ---- k_fa_count -------------------------------------------------------------------------------------------------------------
// What the grammar says of one word: true when the line is not taken for it.  Every byte is a digit, a blank or a tab; a
// terminator has a digit before it (no two separators side by side, none at the line's ends); no four digits in a row; no value
// above 254.
FA_FN bool fa_qbad(const FaQ &q)
{
    bool bad = q.bad != 0;
    bad = bad || (q.term & ~(q.dig << 1)) != 0;
    bad = bad || (q.dig & (q.dig << 1) & (q.dig << 2) & (q.dig << 3) & 0xffff0u) != 0;
#ifndef FA_WRONG_NO_VALUE_CAP                     // (the checker's sensitivity build: 255 and 300 go through)
    uint32_t over = 0;
#pragma unroll
    for (int t = 4; t <= 20; t++) over |= ((q.term >> t) & 1u) & (fa_value(q, t) > 254u ? 1u : 0u);
    bad = bad || over != 0;
#endif
    return bad;
}

// the separators of the word
FA_FN int fa_qseps(const FaQ &q) { return __builtin_popcount(q.sep & 0xffff0u); }

// A lane's share of a record's quality line: words sub, sub + FA_GROUP, ... of it.  -> its separators, *bad: its grammar.
FA_FN int64_t fa_count_lane(const uint8_t *qtext, const FaRec &r, int sub, bool *bad)
{
    int64_t seps = 0;
    bool b = false;
    const int64_t w1 = fa_end_word(r);
    for (int64_t w = fa_first_word(r) + sub; w < w1; w += FA_GROUP) {
        FaQ q;
        fa_qload(qtext, r, w, &q);
        b = b || fa_qbad(q);
        seps += fa_qseps(q);
    }
    *bad = b;
    return seps;
}

// what the group's sums say of a record whose lines were fine: 0, or why it is not taken
FA_FN int fa_verdict(const FaRec &r, bool bad, int64_t seps)
{
    if (bad) return FA_WHY_TOKEN;
    if (seps + 1 != r.seq_len) return FA_WHY_LENGTH;
    return 0;
}

// ---- k_fa_write -------------------------------------------------------------------------------------------------------------
// A lane's share of a run of n bytes at text[a ..) (a checked span), copied to out[at ..): the aligned words sub, sub + FA_GROUP,
// ... that hold it, stored by bytes (the place of a slot is any byte)
template <typename Out>
FA_FN void fa_copy(const uint8_t *text, int64_t a, int64_t n, int sub, Out &o, int64_t at)
{
    if (n <= 0) return;
    const int64_t w1 = ((a + n - 1) >> 4) + 1;
    for (int64_t w = (a >> 4) + sub; w < w1; w += FA_GROUP) {
        const FqWord v = FQ_LDW(text, w);
        const uint32_t x[4] = {v.x, v.y, v.z, v.w};
        const int64_t base = w * FQ_WORD_BYTES;
#pragma unroll
        for (int i = 0; i < FQ_WORD_BYTES; i++) {
            const int64_t p = base + i;
            if (p >= a && p < a + n) FA_ST8(o, at + (p - a), (x[i >> 2] >> (8 * (i & 3))) & 0xffu);
        }
    }
}

// The tokens one word ends, each as one byte at its rank: `before` = the separators of the line before this word (the running
// base of the step plus the exclusive scan of the group's fa_qseps); a token's rank is the number of separators before its
// terminator.  Ranks past the sequence are not stored (k_fa_count refused such a line).
template <typename Out>
FA_FN void fa_qstore(const FaQ &q, const FaRec &r, int64_t before, Out &o, int64_t at)
{
    int64_t rank = before;
#pragma unroll
    for (int t = 4; t <= 20; t++) {
        if ((q.term >> t) & 1u) {
#ifdef FA_WRONG_RANK_BY_BYTES                     // (the checker's sensitivity build: right only while every token is one digit)
            const int64_t k = (q.base + t - r.q_off) >> 1;
#else
            const int64_t k = rank;
#endif
            if (k >= 0 && k < r.seq_len) FA_ST8(o, at + k, fa_value(q, t) & 0xffu);
        }
        rank += (q.sep >> t) & 1u;
    }
}

// the six columns of mio_fasta_qual_index's row for a slot at `at`, and k_pack_text's descriptor over the same buffer
FA_FN void fa_row_out(const FaRec &r, int64_t at, int32_t max_len, int64_t row[6], mpb_text_row *desc)
{
    row[0] = at; row[1] = r.hdr_len;
    row[2] = at + r.hdr_len; row[3] = r.seq_len;
    row[4] = at + r.hdr_len + r.seq_len; row[5] = r.seq_len;
    int64_t pl = r.seq_len;
    if (max_len > 0 && pl > max_len) pl = max_len;           // mio_pack's rule
    desc->seq_off = row[2]; desc->qual_off = row[4]; desc->len = (int32_t)pl; desc->pad = 0;
}
