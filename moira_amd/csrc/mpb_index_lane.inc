// mpb_index_lane.inc -- what ONE LANE of the FASTQ record indexer does (mpb_index_kernels.hip: k_fq_lines, k_fq_starts, k_fq_rows),
// with no wave intrinsic in it, so that a host program runs the same text with checked loads and stores
// (tests/helpers/fastq_index_check.cpp).  The includer defines
//     FQ_FN                        the function qualifier (__device__ __forceinline__ / static inline)
//     FqWord                       four 32-bit words: 16 text bytes, little-endian
//     FQ_LDW(text, w)              the ALIGNED 16-byte word w of the text (bytes 16 w .. 16 w + 15); the allocation holds
//                                  round_up(text_bytes, 16) bytes, and a word is asked for only when 16 w < text_bytes
//     FQ_LDB(text, i)              byte i of the text, asked for only when 0 <= i < text_bytes
//     FQ_LD_START(start, k)        start[k], asked for only when 0 <= k < n_start
//     FQ_ST_START(start, k, v)     start[k] = v, the same
// The rules are mio_fastq_index's (csrc/fastio.cpp), bit for bit; that function is the yardstick and the only code that defines
// an error.  Every loop here runs over the 16 bytes of a word or the bytes of one line.

#define FQ_WORD_BYTES 16
#define FQ_LANES      256                         // lanes of a workgroup of k_fq_lines / k_fq_starts: one word each per trip
#define FQ_TRIPS      4                           // trips of a tile
#define FQ_TILE_WORDS (FQ_LANES * FQ_TRIPS)
#define FQ_TILE       (FQ_TILE_WORDS * FQ_WORD_BYTES)     // T: text bytes per tile (16 KiB)
// a tile's word of the tile table: the newlines in the low 24 bits, then four flags.  HEAD: the byte lies before the tile's last
// newline, so its line is complete whatever follows; TAIL: behind it (the whole tile when it holds no newline), which counts only
// when a later tile holds a newline or the text is final -- the host does not look behind the last newline of a non-final text.
#define FQ_COUNT_MASK    0x00ffffffu
#define FQ_HEAD_NON_ASCII (1u << 24)
#define FQ_HEAD_LONE_CR   (1u << 25)
#define FQ_TAIL_NON_ASCII (1u << 26)
#define FQ_TAIL_LONE_CR   (1u << 27)
// the record kinds (MIO_REC_* of include/moira_io.h, restated: the two libraries stay independent of each other)
#define FQ_REC_OK 0
#define FQ_REC_EMPTY_SEQ 1
#define FQ_REC_EMPTY_QUAL 2
#define FQ_REC_LENGTH_MISMATCH 3

// what str.strip() removes from an ASCII string (fastio.cpp's is_space)
FQ_FN bool fq_is_space(uint32_t c)
{
    return c == 0x20u || (c >= 0x09u && c <= 0x0du) || (c >= 0x1cu && c <= 0x1fu);
}

// One word of the text: bit i of the three masks speaks of byte 16 w + i.  nl: a '\n'; na: a byte >= 0x80; cr: a '\r' that is
// not immediately followed by a '\n' -- the byte after it is READ, from the next word when the '\r' is the word's last byte (and
// a '\r' that is the text's last byte is followed by nothing).  No byte at or past text_bytes sets a bit.
FQ_FN void fq_scan_word(const uint8_t *text, int64_t text_bytes, int64_t w, uint32_t *nl, uint32_t *na, uint32_t *cr)
{
    const int64_t base = w * FQ_WORD_BYTES;
    const FqWord v = FQ_LDW(text, w);
    const uint32_t x[4] = {v.x, v.y, v.z, v.w};
    const int valid = text_bytes - base < FQ_WORD_BYTES ? (int)(text_bytes - base) : FQ_WORD_BYTES;
    uint32_t m_nl = 0, m_na = 0, m_cr = 0;
    for (int i = 0; i < FQ_WORD_BYTES; i++) {
        const uint32_t c = (x[i >> 2] >> (8 * (i & 3))) & 0xffu;
        const uint32_t in = i < valid ? 1u : 0u;
        m_nl |= (in & (c == 0x0au ? 1u : 0u)) << i;
        m_cr |= (in & (c == 0x0du ? 1u : 0u)) << i;
        m_na |= (in & (c >> 7)) << i;
    }
    uint32_t lone = m_cr & ~(m_nl >> 1) & 0x7fffu;           // bytes 0..14: the next byte is in this word (masked: not a '\n')
    if (m_cr & 0x8000u) {
        bool followed = false;
        if (base + FQ_WORD_BYTES < text_bytes) followed = (FQ_LDW(text, w + 1).x & 0xffu) == 0x0au;
        if (!followed) lone |= 0x8000u;
    }
    *nl = m_nl; *na = m_na; *cr = lone;
}

// The tile flags of one word's findings: in_tile = the word's first byte counted from the tile's start, last_nl1 = the position
// of the tile's last newline counted the same way, plus one (0: the tile holds none).
FQ_FN uint32_t fq_word_flags(uint32_t na, uint32_t cr, int in_tile, int last_nl1)
{
    if (!(na | cr)) return 0;
    uint32_t head = 0, tail = 0xffffu;                       // masks of the word's bytes before / behind the last newline
    if (last_nl1 > 0) {
        const int rel = last_nl1 - 1 - in_tile;              // the newline's place in this word (outside 0..15: not in it)
        if (rel >= FQ_WORD_BYTES) { head = 0xffffu; tail = 0; }
        else if (rel >= 0) { head = (1u << rel) - 1u; tail = (0xffffu << (rel + 1)) & 0xffffu; }
    }
    uint32_t f = 0;
    if (na & head) f |= FQ_HEAD_NON_ASCII;
    if (cr & head) f |= FQ_HEAD_LONE_CR;
    if (na & tail) f |= FQ_TAIL_NON_ASCII;
    if (cr & tail) f |= FQ_TAIL_LONE_CR;
    return f;
}

// what a tile's word says once the newlines of the whole text are known: `later` = the text is final, or a newline follows the tile
FQ_FN uint32_t fq_tile_refusal(uint32_t info, bool later)
{
    uint32_t f = info & (FQ_HEAD_NON_ASCII | FQ_HEAD_LONE_CR);
    if (later) f |= (info & (FQ_TAIL_NON_ASCII | FQ_TAIL_LONE_CR)) >> 2;
    return f >> 24;                                          // bit 0: a non-ASCII byte, bit 1: a lone carriage return
}

// The line starts one word gives: the newline at byte p that ends line L stores start[L + 1] = p + 1; line0 = the number of the
// line that the word's first newline ends.  Only entries below n_start are stored.
FQ_FN void fq_store_starts(uint32_t *start, int64_t n_start, int64_t w, uint32_t nl, int64_t line0)
{
    int64_t L = line0;
    for (int i = 0; i < FQ_WORD_BYTES; i++) {
        if (!(nl & (1u << i))) continue;
        if (L + 1 < n_start) FQ_ST_START(start, L + 1, (uint32_t)(w * FQ_WORD_BYTES + i + 1));
        L++;
    }
}

// [a, b) stripped at both ends -> *off, *len (fastio.cpp's strip: an all-blank line's span is {b, 0})
FQ_FN void fq_strip(const uint8_t *text, int64_t a, int64_t b, int64_t *off, int64_t *len)
{
    while (a < b && fq_is_space(FQ_LDB(text, a))) a++;
    while (b > a && fq_is_space(FQ_LDB(text, b - 1))) b--;
    *off = a; *len = b - a;
}

// Record r from start[4 r .. 4 r + 4]: the six columns of mio_fastq_index's row, the record's kind, and k_pack_text's
// descriptor {seq_off, qual_off, min(qual_len, max_len)}.  start[] is device-written and not trusted: returns false, with
// nothing stored, unless every line satisfies 0 <= start < next start <= text_bytes (a line holds its newline, or -- the
// unterminated last line of a final text -- at least one byte).
FQ_FN bool fq_row(const uint8_t *text, int64_t text_bytes, const uint32_t *start, int64_t n_start, int64_t r, int32_t max_len,
                  int64_t row[6], int32_t *kind, mpb_text_row *desc)
{
    if (r < 0 || 4 * r + 4 >= n_start) return false;
    int64_t s[5];
    for (int k = 0; k < 5; k++) s[k] = (int64_t)FQ_LD_START(start, 4 * r + k);
    for (int k = 0; k < 4; k++)
        if (s[k] >= s[k + 1]) return false;
    if (s[4] > text_bytes) return false;
    int64_t off[4], len[4];
    for (int k = 0; k < 4; k++) {
        if (k == 2) continue;                                // the '+' line: whatever it holds
        int64_t e = s[k + 1];
        if (FQ_LDB(text, e - 1) == 0x0au) e--;               // (otherwise: the unterminated last line, which ends at the text's end)
        fq_strip(text, s[k], e, &off[k], &len[k]);
    }
    // header: replace('\t', ' ').split(' ')[0].lstrip('@')
    int64_t h0 = off[0], h1 = h0;
    const int64_t hend = off[0] + len[0];
    while (h1 < hend) {
        const uint32_t c = FQ_LDB(text, h1);
        if (c == 0x20u || c == 0x09u) break;
        h1++;
    }
    while (h0 < h1 && FQ_LDB(text, h0) == 0x40u) h0++;
    row[0] = h0; row[1] = h1 - h0; row[2] = off[1]; row[3] = len[1]; row[4] = off[3]; row[5] = len[3];
    int bad = FQ_REC_OK;                                     // in this order
    if (len[1] == 0) bad = FQ_REC_EMPTY_SEQ;
    else if (len[3] == 0) bad = FQ_REC_EMPTY_QUAL;
    else if (len[1] != len[3]) bad = FQ_REC_LENGTH_MISMATCH;
    *kind = bad;
    int64_t pl = len[3];
    if (max_len > 0 && pl > max_len) pl = max_len;           // mio_pack's rule
    desc->seq_off = off[1]; desc->qual_off = off[3]; desc->len = (int32_t)pl; desc->pad = 0;
    return true;
}
