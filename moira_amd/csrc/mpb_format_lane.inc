// mpb_format_lane.inc -- what ONE LANE of the output formatter does (mpb_format_kernels.hip: k_fmt_count, k_fmt_write), with no
// wave intrinsic in it: a neighbour's count or a place inside the record is an argument, so that a host program runs the same
// text with checked loads and stores (tests/helpers/format_lane_check.cpp).  The step stands between a text with its record
// index and the output files: records sel[k] of the index become fasta, qual or fastq text.
// The rules are mio_format's and mio_format_report's, with put_quals and put_qual_string as they are written (csrc/fastio.cpp); that function
// is the yardstick and the only code that defines the output.  One point of it is easy to miss: with out_offset ==
// fastq_offset the host copies the quality line and turns only the byte fastq_offset itself into fastq_offset + 1 (clamp_q0), so
// a byte BELOW fastq_offset (q < 0) stays as it is there, while with different offsets it is raised to the floor.  fm_qchar
// does the same.
// The includer defines
//     FM_FN                        the function qualifier (__device__ __forceinline__ / static inline)
//     FM_LD_I64(p, k)              p[k] of an int64 array (the index, sel, relabel_index), asked for only inside its rows
//     FM_LD_I32(p, k)              ... of an int32 array (label_id)
//     FM_LD16(text, off)           the aligned 16 bytes at text + off (off % 16 == 0) as an fm_w16, asked for only when a byte of a
//                                  validated range lies in them: below round_up(text_bytes, 16) for the text, inside the blob
//     FM_ST8(o, pos, byte)         one byte of the output at position pos of the whole formatted text; o is an FmOut
//     FM_LD_U64(p, k)              optional: the 64 bits of p[k] of the ee array (k < nsel).  With it the file also gives fm_rec_row,
//                                  the row check of mpb_format_records_host (the report kind, the ee suffix, aux); FM_LD_I32 then
//                                  also serves the three aux arrays, asked for only at a record inside 0 .. n_records - 1
// Every loop here runs over a checked length or a fixed table.

#define FM_LANES 256                              // lanes of a workgroup of k_fmt_count / k_fmt_write
#define FM_GROUP 8                                // lanes that share one record, as in k_pack_text
#define FM_KIND_FASTA 0                           // MIO_FMT_FASTA / _QUAL / _FASTQ
#define FM_KIND_QUAL  1
#define FM_KIND_FASTQ 2
#define FM_KIND_REPORT 4                          // MIO_FMT_REPORT: a contigs.report line (3 is the collapse's names line: not here)
#define FM_SFX_MAX 32                             // bytes of ";ee=%.2f;size=1;" inside the taken domain
#define FM_MAX_LABELS 16
#define FM_STR_MAX 255                            // bytes of relabel and of a label
#define FM_SLOT 256                               // the blob: relabel in slot 0, label i in slot 1 + i, zero filled
#define FM_BLOB_BYTES ((FM_MAX_LABELS + 1) * FM_SLOT)

struct fm_w16 { uint32_t w[4]; };

// what a call formats by; travels by value (the strings lie in the blob)
struct FmParams {
    int64_t n_records, text_bytes;
    int32_t kind, fastq_offset, out_offset, floor_q, max_len;
    int32_t has_relabel, has_labels, n_labels;
    uint8_t str_len[FM_MAX_LABELS + 1];           // [0] relabel, [1 + i] label i
    int32_t has_ee, aux_stride;                   // ee[k] by position; aux: element r * aux_stride of each of three arrays, by record
};

// a selected record after every check: the ranges lie inside the text
struct FmRow {
    int64_t hdr_off, seq_off, qual_off, relabel_index;
    int32_t hdr_len, L, label;                    // L: min(SEQ_LEN, max_len); label: -1 for none
};

// what a record carries beyond its row: the ee suffix (sfx_len == 0: none) and the report line's three numbers
struct FmExtra {
    uint64_t q;                                   // |ee| in hundredths, rounded as "%.2f" rounds
    int32_t neg, sfx_len;
    int32_t aux[3];
};

FM_FN void fm_extra_none(FmExtra *x) { x->q = 0; x->neg = 0; x->sfx_len = 0; x->aux[0] = 0; x->aux[1] = 0; x->aux[2] = 0; }

// Row sel[k] of the index by every check (the row is not trusted, wherever it comes from).  false: nothing of it may be read.
FM_FN bool fm_row(const int64_t *idx, const int64_t *sel, const int64_t *relabel_index, const int32_t *label_id, int64_t k,
                  const FmParams &p, FmRow *o)
{
    o->hdr_off = 0; o->seq_off = 0; o->qual_off = 0; o->relabel_index = 0; o->hdr_len = 0; o->L = 0; o->label = -1;
    const int64_t r = sel ? FM_LD_I64(sel, k) : k;
    if (r < 0 || r >= p.n_records) return false;
    // (the row lies inside the index, entry k inside the per-record arrays: every word is loaded, then every check is made -- one
    // verdict, one way out)
    const int64_t ho = FM_LD_I64(idx, r * 6 + 0), hl = FM_LD_I64(idx, r * 6 + 1);
    const int64_t so = FM_LD_I64(idx, r * 6 + 2), sl = FM_LD_I64(idx, r * 6 + 3);
    const bool quals = p.kind != FM_KIND_FASTA;
    const int64_t qo = quals ? FM_LD_I64(idx, r * 6 + 4) : 0, ql = quals ? FM_LD_I64(idx, r * 6 + 5) : sl;
    const int64_t ri = p.has_relabel ? FM_LD_I64(relabel_index, k) : 0;
    const int32_t lab = p.has_labels ? FM_LD_I32(label_id, k) : -1;
    bool ok = ho >= 0 && hl >= 0 && hl <= 0x7fffffffll && hl <= p.text_bytes && ho <= p.text_bytes - hl;
    ok = ok && so >= 0 && sl >= 0 && sl <= 0x7fffffffll && sl <= p.text_bytes && so <= p.text_bytes - sl;
    ok = ok && ql == sl && qo >= 0 && qo <= p.text_bytes - sl;
    ok = ok && ri >= 0 && lab < p.n_labels;
    if (!ok) return false;
    o->hdr_off = ho; o->seq_off = so; o->qual_off = qo; o->relabel_index = ri;
    o->hdr_len = (int32_t)hl; o->label = lab < 0 ? -1 : lab;
    o->L = (int32_t)(p.max_len > 0 && sl > p.max_len ? p.max_len : sl);
    return true;
}

// the decimal digits of v >= 0 (1..19)
FM_FN int fm_digits(int64_t v)
{
    uint64_t p = 10;
    int nd = 1;
    for (; nd < 19 && (uint64_t)v >= p; nd++) p *= 10;
    return nd;
}

// the value put_quals prints for a quality byte, 0..255
FM_FN int fm_qval(uint32_t b, const FmParams &p)
{
    const int q = (int)b - p.fastq_offset;
    return q <= p.floor_q ? p.floor_q : q > 255 ? 255 : q;
}

// the character put_qual_string writes for a quality byte (see the head of this file for the equal-offset form)
FM_FN uint32_t fm_qchar(uint32_t b, const FmParams &p)
{
#ifdef FM_WRONG_UPPER_CLAMP                       // (the checker's sensitivity build: a clamp the host does not have)
    { const int q0 = (int)b - p.fastq_offset; if (q0 > 41) return (uint32_t)(41 + p.out_offset) & 255u; }
#endif
    if (p.out_offset == p.fastq_offset) return (p.floor_q > 0 && b == (uint32_t)p.fastq_offset) ? (b + 1u) & 255u : b;
    int q = (int)b - p.fastq_offset;
    q = q <= p.floor_q ? p.floor_q : q;
    return (uint32_t)(q + p.out_offset) & 255u;
}

FM_FN uint32_t fm_byte(const fm_w16 &v, int t) { return (v.w[t >> 2] >> (8 * (t & 3))) & 255u; }

// bytes [sh, sh + 16) of the 32 bytes a | b, sh = 0..15 (k_pack_text's funnel, in plain C)
FM_FN fm_w16 fm_funnel16(const fm_w16 &a, const fm_w16 &b, uint32_t sh)
{
    uint32_t w0 = a.w[0], w1 = a.w[1], w2 = a.w[2], w3 = a.w[3], w4 = b.w[0], w5 = b.w[1];
    if (sh & 8u) { w0 = a.w[2]; w1 = a.w[3]; w2 = b.w[0]; w3 = b.w[1]; w4 = b.w[2]; w5 = b.w[3]; }
    if (sh & 4u) { w0 = w1; w1 = w2; w2 = w3; w3 = w4; w4 = w5; }
    const uint32_t bs = 8u * (sh & 3u);
    fm_w16 o;
    o.w[0] = (uint32_t)((((uint64_t)w1 << 32) | w0) >> bs);
    o.w[1] = (uint32_t)((((uint64_t)w2 << 32) | w1) >> bs);
    o.w[2] = (uint32_t)((((uint64_t)w3 << 32) | w2) >> bs);
    o.w[3] = (uint32_t)((((uint64_t)w4 << 32) | w3) >> bs);
    return o;
}

// the 16 bytes at text[s ..), of which the first m (1..16) lie in a validated range: s + m <= text_bytes, so the aligned word of s
// ends below round_up(text_bytes, 16), and so does the next one whenever one of the m bytes lies in it
FM_FN fm_w16 fm_fetch16(const uint8_t *text, int64_t s, int m)
{
    const int64_t base = s & ~(int64_t)15;
    const uint32_t sh = (uint32_t)(s & 15);
    const fm_w16 a = FM_LD16(text, base);
    fm_w16 b;
    b.w[0] = 0; b.w[1] = 0; b.w[2] = 0; b.w[3] = 0;
    if (sh + (uint32_t)m > 16u) b = FM_LD16(text, base + 16);
    return fm_funnel16(a, b, sh);
}

// ---- k_fmt_count ------------------------------------------------------------------------------------------------------------
// the values >= 10 and >= 100 among the first nv (<= 16) quality bytes of a word, after the clamp: n10 | n100 << 32
FM_FN uint64_t fm_count16(const fm_w16 &ql, int nv, const FmParams &p)
{
    uint64_t c = 0;
#pragma unroll
    for (int t = 0; t < 16; t++) {
        const int v = fm_qval(fm_byte(ql, t), p);
        if (t < nv) c += (v >= 10 ? 1ull : 0ull) + (v >= 100 ? 1ull << 32 : 0ull);
    }
    return c;
}

// a lane's share of a QUAL record's counts: chunks sub, sub + FM_GROUP, ... of the quality line
FM_FN uint64_t fm_count_lane(const uint8_t *text, const FmRow &r, int sub, const FmParams &p)
{
    uint64_t c = 0;
    for (int64_t at = 16 * (int64_t)sub; at < r.L; at += 16 * FM_GROUP) {
        const int nv = r.L - at < 16 ? (int)(r.L - at) : 16;
        c += fm_count16(fm_fetch16(text, r.qual_off + at, nv), nv, p);
    }
    return c;
}

// ---- "%.2f" and "%d" in integers --------------------------------------------------------------------------------------------
// The 64 bits of a double -> its hundredths as snprintf("%.2f") rounds them: half-even on the exact binary value.  false: not
// finite, or |x| >= 2^53 (outside the taken domain; the caller formats on the host).  x = m 2^-s, m < 2^53, s >= 0; t = 100 m
// < 2^60; q = t >> s, rounded up when the s low bits are above the half, or are the half and q is odd.  The sign is the sign
// bit: -0.0 and -0.001 print "-0.00", as glibc prints them.
FM_FN bool fm_ee_q(uint64_t bits, uint64_t *q, int32_t *neg)
{
    const int e = (int)((bits >> 52) & 0x7ffu);
    const uint64_t frac = bits & ((1ull << 52) - 1);
    *neg = (int32_t)(bits >> 63);
    *q = 0;
    if (e > 1075) return false;                   // 1075: [2^52, 2^53); 2047: inf and NaN
    const uint64_t m = e ? frac | (1ull << 52) : frac;
    const int s = 1075 - (e ? e : 1);
    const uint64_t t = 100 * m;
    if (s == 0) { *q = t; return true; }
    if (s >= 64) return true;
    uint64_t v = t >> s;
    const uint64_t rem = t & ((1ull << s) - 1), half = 1ull << (s - 1);
#ifdef FM_WRONG_TIES_HALF_UP                      // (the checker's sensitivity build: ties away from zero)
    if (rem >= half) v++;
#else
    if (rem > half || (rem == half && (v & 1))) v++;
#endif
    *q = v;
    return true;
}

// bytes of ";ee=" [-] digits "." 2 digits ";size=1;"
FM_FN int fm_sfx_bytes(uint64_t q, int32_t neg) { return 4 + (neg ? 1 : 0) + fm_digits((int64_t)(q / 100)) + 3 + 8; }

// bytes of "%d"
FM_FN int fm_i32_bytes(int32_t v)
{
#ifdef FM_WRONG_AUX_SIGN                          // (the checker's sensitivity build: the magnitude alone)
    return fm_digits((int64_t)(v < 0 ? 0u - (uint32_t)v : (uint32_t)v));
#else
    return (v < 0 ? 1 : 0) + fm_digits((int64_t)(v < 0 ? 0u - (uint32_t)v : (uint32_t)v));
#endif
}

// bytes of "\t1\t%d\t%d\t%d\n"
FM_FN int fm_report_tail_bytes(const FmExtra &x) { return 6 + fm_i32_bytes(x.aux[0]) + fm_i32_bytes(x.aux[1]) + fm_i32_bytes(x.aux[2]); }

// bytes of the header line, the newline included (REPORT: of the whole line)
FM_FN int64_t fm_header_bytes_x(const FmRow &r, const FmExtra &x, const FmParams &p)
{
    int64_t n = (p.has_relabel ? (int64_t)p.str_len[0] + fm_digits(r.relabel_index) : (int64_t)r.hdr_len) + x.sfx_len;
    if (p.kind == FM_KIND_REPORT) return n + fm_report_tail_bytes(x);
    if (r.label >= 0) n += 1 + (int64_t)p.str_len[1 + r.label];
    return n + 2;
}

FM_FN int64_t fm_header_bytes(const FmRow &r, const FmParams &p)
{
    FmExtra x;
    fm_extra_none(&x);
    return fm_header_bytes_x(r, x, p);
}

// the output bytes of a record; counts: the record's n10 | n100 << 32 (QUAL only)
FM_FN int64_t fm_size_x(const FmRow &r, const FmExtra &x, uint64_t counts, const FmParams &p)
{
    const int64_t h = fm_header_bytes_x(r, x, p), L = r.L;
    if (p.kind == FM_KIND_REPORT) return h;
    if (p.kind == FM_KIND_FASTA) return h + L + 1;
    if (p.kind == FM_KIND_FASTQ) return h + L + 3 + L + 1;
    if (L == 0) return h + 1;
    return h + L + (int64_t)(counts & 0xffffffffull) + (int64_t)(counts >> 32) + (L - 1) + 1;
}

FM_FN int64_t fm_size(const FmRow &r, uint64_t counts, const FmParams &p)
{
    FmExtra x;
    fm_extra_none(&x);
    return fm_size_x(r, x, counts, p);
}

// ---- k_fmt_write ------------------------------------------------------------------------------------------------------------
#define FM_COPY   0                               // what a moved byte becomes: itself
#define FM_HEADER 1                               // ... ':' -> '_'
#define FM_QCHAR  2                               // ... fm_qchar

// A lane's share of a run of n bytes at text[src ..) (a validated range, or a slot of the blob), moved to the output at `at`:
// chunks sub, sub + FM_GROUP, ... of 16 bytes, each fetched as aligned words and funnelled, then stored by bytes (the place of a
// record in the output is any byte: DESIGN 4o)
template <typename Out>
FM_FN void fm_move(const uint8_t *text, int64_t src, int64_t n, int how, int sub, const FmParams &p, Out &o, int64_t at)
{
    for (int64_t c = 16 * (int64_t)sub; c < n; c += 16 * FM_GROUP) {
        const int m = n - c < 16 ? (int)(n - c) : 16;
        const fm_w16 v = fm_fetch16(text, src + c, m);
#pragma unroll
        for (int t = 0; t < 16; t++) {
            uint32_t b = fm_byte(v, t);
            if (how == FM_HEADER) b = b == (uint32_t)':' ? (uint32_t)'_' : b;
            if (how == FM_QCHAR) b = fm_qchar(b, p);
            if (t < m) FM_ST8(o, at + c + t, b);
        }
    }
}

// the decimal digits of v (nd of them) at `at`, by one lane
template <typename Out>
FM_FN void fm_put_digits(uint64_t v, int nd, Out &o, int64_t at)
{
    for (int i = nd - 1; i >= 0; i--) { FM_ST8(o, at + i, (uint32_t)('0' + (int)(v % 10))); v /= 10; }
}

// ";ee=%.2f;size=1;" at `at`, by one lane
template <typename Out>
FM_FN void fm_put_sfx(const FmExtra &x, Out &o, int64_t at)
{
    int64_t w = at;
    FM_ST8(o, w, (uint32_t)';'); FM_ST8(o, w + 1, (uint32_t)'e'); FM_ST8(o, w + 2, (uint32_t)'e'); FM_ST8(o, w + 3, (uint32_t)'=');
    w += 4;
    if (x.neg) { FM_ST8(o, w, (uint32_t)'-'); w++; }
    const uint64_t ip = x.q / 100;
    const int nd = fm_digits((int64_t)ip), fr = (int)(x.q % 100);
    fm_put_digits(ip, nd, o, w);
    w += nd;
    FM_ST8(o, w, (uint32_t)'.'); FM_ST8(o, w + 1, (uint32_t)('0' + fr / 10)); FM_ST8(o, w + 2, (uint32_t)('0' + fr % 10));
    w += 3;
    FM_ST8(o, w, (uint32_t)';'); FM_ST8(o, w + 1, (uint32_t)'s'); FM_ST8(o, w + 2, (uint32_t)'i'); FM_ST8(o, w + 3, (uint32_t)'z');
    FM_ST8(o, w + 4, (uint32_t)'e'); FM_ST8(o, w + 5, (uint32_t)'='); FM_ST8(o, w + 6, (uint32_t)'1'); FM_ST8(o, w + 7, (uint32_t)';');
}

// "\t1\t%d\t%d\t%d\n" at `at`, by one lane
template <typename Out>
FM_FN void fm_put_report_tail(const FmExtra &x, Out &o, int64_t at)
{
    int64_t w = at;
    FM_ST8(o, w, (uint32_t)'\t'); FM_ST8(o, w + 1, (uint32_t)'1');
    w += 2;
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const int32_t v = x.aux[j];
        const uint32_t mag = v < 0 ? 0u - (uint32_t)v : (uint32_t)v;
        FM_ST8(o, w, (uint32_t)'\t'); w++;
#ifndef FM_WRONG_AUX_SIGN
        if (v < 0) { FM_ST8(o, w, (uint32_t)'-'); w++; }
#endif
        const int nd = fm_digits((int64_t)mag);
        fm_put_digits((uint64_t)mag, nd, o, w);
        w += nd;
    }
    FM_ST8(o, w, (uint32_t)'\n');
}

// the header line of a record at `at` (REPORT: the whole line), by the lanes of its group; -> its bytes
template <typename Out>
FM_FN int64_t fm_write_header_x(const uint8_t *text, const uint8_t *blob, const FmRow &r, const FmExtra &x, int sub, const FmParams &p,
                                Out &o, int64_t at)
{
    int64_t w = at;
    if (p.kind != FM_KIND_REPORT) {
        if (sub == 0) FM_ST8(o, w, p.kind == FM_KIND_FASTQ ? (uint32_t)'@' : (uint32_t)'>');
        w++;
    }
    if (p.has_relabel) {
        fm_move(blob, 0, (int64_t)p.str_len[0], FM_COPY, sub, p, o, w);
        w += p.str_len[0];
        const int nd = fm_digits(r.relabel_index);
        if (sub == FM_GROUP - 1) fm_put_digits((uint64_t)r.relabel_index, nd, o, w);   // (the lane with the least to move of a short string)
        w += nd;
    } else {
        fm_move(text, r.hdr_off, (int64_t)r.hdr_len, FM_HEADER, sub, p, o, w);
        w += r.hdr_len;
    }
    if (x.sfx_len > 0) {
        if (sub == FM_GROUP - 2) fm_put_sfx(x, o, w);
        w += x.sfx_len;
    }
    if (p.kind == FM_KIND_REPORT) {
        if (sub == FM_GROUP - 3) fm_put_report_tail(x, o, w);
        return w + fm_report_tail_bytes(x) - at;
    }
    if (r.label >= 0) {
        if (sub == 0) FM_ST8(o, w, (uint32_t)'\t');
        w++;
        fm_move(blob, (int64_t)(1 + r.label) * FM_SLOT, (int64_t)p.str_len[1 + r.label], FM_COPY, sub, p, o, w);
        w += p.str_len[1 + r.label];
    }
    if (sub == 0) FM_ST8(o, w, (uint32_t)'\n');
    return w + 1 - at;
}

template <typename Out>
FM_FN int64_t fm_write_header(const uint8_t *text, const uint8_t *blob, const FmRow &r, int sub, const FmParams &p, Out &o, int64_t at)
{
    FmExtra x;
    fm_extra_none(&x);
    return fm_write_header_x(text, blob, r, x, sub, p, o, at);
}

// everything of a FASTA or FASTQ record behind its header line, at `at`
template <typename Out>
FM_FN void fm_write_lines(const uint8_t *text, const FmRow &r, int sub, const FmParams &p, Out &o, int64_t at)
{
    const int64_t L = r.L;
    fm_move(text, r.seq_off, L, FM_COPY, sub, p, o, at);
    if (sub == 1) FM_ST8(o, at + L, (uint32_t)'\n');
    if (p.kind != FM_KIND_FASTQ) return;
    if (sub == 1) { FM_ST8(o, at + L + 1, (uint32_t)'+'); FM_ST8(o, at + L + 2, (uint32_t)'\n'); }
    fm_move(text, r.qual_off, L, FM_QCHAR, sub, p, o, at + L + 3);
    if (sub == 2) FM_ST8(o, at + 2 * L + 3, (uint32_t)'\n');
}

// QUAL.  Step s of a record's group: lane `sub` owns values [16 (s FM_GROUP + sub), + 16).  Its bytes: every value's digits and
// one blank in front of each but the record's first.
FM_FN int fm_qual_bytes16(const fm_w16 &ql, int nv, bool first, const FmParams &p)
{
    if (nv <= 0) return 0;
    const uint64_t c = fm_count16(ql, nv, p);
    return 2 * nv + (int)(c & 0xffffffffull) + (int)(c >> 32) - (first ? 1 : 0);
}

// ... rendered at `at` (the running base of the step plus the exclusive scan of the lanes' fm_qual_bytes16 before this one)
template <typename Out>
FM_FN void fm_qual_render16(const fm_w16 &ql, int nv, bool first, const FmParams &p, Out &o, int64_t at)
{
    int64_t w = at;
#pragma unroll
    for (int t = 0; t < 16; t++) {
        if (t < nv) {
            const int v = fm_qval(fm_byte(ql, t), p);
            if (!(first && t == 0)) { FM_ST8(o, w, (uint32_t)' '); w++; }
            const int h = v / 100, d = (v / 10) % 10;
            if (v >= 100) { FM_ST8(o, w, (uint32_t)('0' + h)); w++; }
            if (v >= 10) { FM_ST8(o, w, (uint32_t)('0' + d)); w++; }
            FM_ST8(o, w, (uint32_t)('0' + v % 10)); w++;
        }
    }
#ifdef FM_WRONG_TRAILING_BLANK                    // (the checker's sensitivity build: ' '.join has no blank behind the last value)
    if (nv > 0) FM_ST8(o, w, (uint32_t)' ');
#endif
}

// the lane's quality word of step s (nv <= 0: none, nothing is fetched); *nv: its values
FM_FN fm_w16 fm_qual_word(const uint8_t *text, const FmRow &r, int step, int sub, int *nv)
{
    const int64_t at = 16 * ((int64_t)step * FM_GROUP + sub);
    const int64_t left = (int64_t)r.L - at;
    fm_w16 v;
    v.w[0] = 0; v.w[1] = 0; v.w[2] = 0; v.w[3] = 0;
    *nv = left >= 16 ? 16 : left > 0 ? (int)left : 0;
    if (*nv > 0) v = fm_fetch16(text, r.qual_off + at, *nv);
    return v;
}

// ---- mpb_format_records_host's row ------------------------------------------------------------------------------------------------
#ifdef FM_LD_U64
// Row sel[k] with what the record carries beyond it.  Kinds 0..2: fm_row's checks; REPORT: sel, the header's range, relabel_index
// -- the sequence and quality columns are neither read nor checked, and there is no label -- then aux by RECORD (r inside
// 0 .. n_records - 1 by then).  ee by POSITION k, finite and below 2^53 or the row fails.  false: nothing of it may be read.
FM_FN bool fm_rec_row(const int64_t *idx, const int64_t *sel, const int64_t *relabel_index, const int32_t *label_id, const uint64_t *ee,
                      const int32_t *aux0, const int32_t *aux1, const int32_t *aux2, int64_t k, const FmParams &p, FmRow *o, FmExtra *x)
{
    fm_extra_none(x);
    bool ok;
    if (p.kind != FM_KIND_REPORT) {
        ok = fm_row(idx, sel, relabel_index, label_id, k, p, o);
    } else {
        o->hdr_off = 0; o->seq_off = 0; o->qual_off = 0; o->relabel_index = 0; o->hdr_len = 0; o->L = 0; o->label = -1;
        const int64_t r = sel ? FM_LD_I64(sel, k) : k;
        if (r < 0 || r >= p.n_records) return false;
        const int64_t ho = FM_LD_I64(idx, r * 6 + 0), hl = FM_LD_I64(idx, r * 6 + 1);
        const int64_t ri = p.has_relabel ? FM_LD_I64(relabel_index, k) : 0;
        x->aux[0] = FM_LD_I32(aux0, r * p.aux_stride); x->aux[1] = FM_LD_I32(aux1, r * p.aux_stride);
        x->aux[2] = FM_LD_I32(aux2, r * p.aux_stride);
        ok = ho >= 0 && hl >= 0 && hl <= 0x7fffffffll && hl <= p.text_bytes && ho <= p.text_bytes - hl && ri >= 0;
        if (ok) { o->hdr_off = ho; o->hdr_len = (int32_t)hl; o->relabel_index = ri; }
    }
    if (p.has_ee) {
        const bool in_domain = fm_ee_q(FM_LD_U64(ee, k), &x->q, &x->neg);
        ok = ok && in_domain;
        x->sfx_len = ok ? fm_sfx_bytes(x->q, x->neg) : 0;
    }
    return ok;
}
#endif
