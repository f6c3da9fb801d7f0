// Host twin of the device FASTQ indexer (moira_amd/csrc/mpb_index_kernels.hip): the per-lane code of
// moira_amd/csrc/mpb_index_lane.inc compiled for the host and run as the four kernels run it -- workgroups of 256 lane states
// (four waves of 64) that take every step in lockstep, the workgroup's own parts (sum, last newline, scan of the counts) done
// between the steps -- followed by the host entry's decisions (csrc/mpb_index.cpp).  The text lies in a heap block of exactly
// round_up(text_bytes, 16) bytes whose padding holds newlines, carriage returns and bytes >= 0x80; the line table and the rows lie
// in blocks of exactly their size.  Every load and store goes through an accessor that checks the position: one outside its
// block is counted, not made, and fails the run (exit status 3).  tests/test_fastq_index_lane_model.py builds this program with
// the address and undefined-behaviour sanitizers, together with csrc/fastio.cpp, and every case is compared here with
// mio_fastq_index: a text that is taken must give its n, consumed, bad_kind and rows [0, n + (bad_kind ? 1 : 0)); a text the host
// calls unsupported must not be taken.
//
// Input (argv[1]): little-endian  int32 cases;  per case  int64 text_bytes, max_records;  int32 final, max_len;  the text.
// Output (argv[2]): per case  int32 why, bad_kind;  int64 n, consumed, longest;  int32 host_rc (0, or MIO_E_*), pad.
// Prints "<cases> texts, <t> taken, <o> loads or stores out of bounds, <d> differ from mio_fastq_index, <u> unsupported texts taken".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "moira_io.h"
#include "moira_pb.h"

static int64_t g_text_bytes = 0, g_text_cap = 0, g_n_start = 0;
static long g_oob = 0;

struct FqWord { uint32_t x, y, z, w; };
#define FQ_FN static inline
static inline FqWord fq_ldw(const uint8_t *text, int64_t w)
{
    FqWord v = {0, 0, 0, 0};
    if (w < 0 || w * 16 >= g_text_bytes || w * 16 + 16 > g_text_cap) { g_oob++; return v; }
    memcpy(&v, text + w * 16, 16);
    return v;
}
static inline uint32_t fq_ldb(const uint8_t *text, int64_t i)
{
    if (i < 0 || i >= g_text_bytes) { g_oob++; return 0; }
    return text[i];
}
static inline uint32_t fq_ld_start(const uint32_t *start, int64_t k)
{
    if (k < 0 || k >= g_n_start) { g_oob++; return 0; }
    return start[k];
}
static inline void fq_st_start(uint32_t *start, int64_t k, uint32_t v)
{
    if (k < 0 || k >= g_n_start) { g_oob++; return; }
    start[k] = v;
}
#define FQ_LDW(text, w) fq_ldw((text), (w))
#define FQ_LDB(text, i) fq_ldb((text), (i))
#define FQ_LD_START(start, k) fq_ld_start((start), (k))
#define FQ_ST_START(start, k, v) fq_st_start((start), (k), (v))
#include "mpb_index_lane.inc"

static_assert(FQ_REC_EMPTY_SEQ == MIO_REC_EMPTY_SEQ && FQ_REC_EMPTY_QUAL == MIO_REC_EMPTY_QUAL &&
              FQ_REC_LENGTH_MISMATCH == MIO_REC_LENGTH_MISMATCH && MPB_IDX_COLS == MIO_IDX_COLS, "the restated constants");

struct Result { int32_t why = 0, bad_kind = 0; int64_t n = 0, consumed = 0, longest = 0; std::vector<int64_t> rows; };

// k_fq_lines for one tile
static uint32_t model_lines(const uint8_t *text, int64_t text_bytes, int64_t tile)
{
    uint32_t na[FQ_LANES][FQ_TRIPS], cr[FQ_LANES][FQ_TRIPS], count[FQ_LANES];
    int last[FQ_LANES];
    for (int tid = 0; tid < FQ_LANES; tid++) { count[tid] = 0; last[tid] = 0; }
    for (int t = 0; t < FQ_TRIPS; t++)                       // (a trip is one step of every lane)
        for (int tid = 0; tid < FQ_LANES; tid++) {
            const int in_tile = (t * FQ_LANES + tid) * FQ_WORD_BYTES;
            const int64_t w = tile * FQ_TILE_WORDS + t * FQ_LANES + tid;
            uint32_t nl = 0;
            na[tid][t] = 0; cr[tid][t] = 0;
            if (w * FQ_WORD_BYTES < text_bytes) fq_scan_word(text, text_bytes, w, &nl, &na[tid][t], &cr[tid][t]);
            count[tid] += (uint32_t)__builtin_popcount(nl);
            if (nl) last[tid] = in_tile + (32 - __builtin_clz(nl));
        }
    uint32_t sum = 0, flags = 0;
    int last_nl1 = 0;
    for (int tid = 0; tid < FQ_LANES; tid++) { sum += count[tid]; if (last[tid] > last_nl1) last_nl1 = last[tid]; }
    for (int tid = 0; tid < FQ_LANES; tid++)
        for (int t = 0; t < FQ_TRIPS; t++) flags |= fq_word_flags(na[tid][t], cr[tid][t], (t * FQ_LANES + tid) * FQ_WORD_BYTES, last_nl1);
    return sum | flags;
}

// k_fq_starts for one tile
static void model_starts(const uint8_t *text, int64_t text_bytes, int64_t tile, uint32_t prefix, uint32_t newlines, uint32_t lines,
                         uint32_t *start, int64_t n_start)
{
    int64_t line = prefix;
    if (tile == 0) {
        if (n_start > 0) FQ_ST_START(start, 0, 0u);
        if (lines > newlines && (int64_t)lines < n_start) FQ_ST_START(start, lines, (uint32_t)text_bytes);
    }
    if (line + 1 >= n_start) return;
    for (int t = 0; t < FQ_TRIPS; t++) {
        uint32_t nl[FQ_LANES], rank[FQ_LANES], run = 0;
        for (int tid = 0; tid < FQ_LANES; tid++) {
            const int64_t w = tile * FQ_TILE_WORDS + t * FQ_LANES + tid;
            uint32_t na, cr;
            nl[tid] = 0;
            if (w * FQ_WORD_BYTES < text_bytes) fq_scan_word(text, text_bytes, w, &nl[tid], &na, &cr);
        }
        for (int tid = 0; tid < FQ_LANES; tid++) { rank[tid] = run; run += (uint32_t)__builtin_popcount(nl[tid]); }     // the workgroup's scan
        for (int tid = 0; tid < FQ_LANES; tid++)
            if (nl[tid]) fq_store_starts(start, n_start, tile * FQ_TILE_WORDS + t * FQ_LANES + tid, nl[tid], line + rank[tid]);
        line += run;
    }
}

static Result model(const uint8_t *text, int64_t text_bytes, int final_text, int64_t max_records, int32_t max_len)
{
    Result R;
    const int64_t n_tiles = (text_bytes + FQ_TILE - 1) / FQ_TILE;
    std::vector<uint32_t> info((size_t)n_tiles), prefix((size_t)n_tiles);
    for (int64_t t = 0; t < n_tiles; t++) info[(size_t)t] = model_lines(text, text_bytes, t);
    // k_fq_scan
    uint32_t total = 0;
    for (int64_t t = 0; t < n_tiles; t++) { prefix[(size_t)t] = total; total += info[(size_t)t] & FQ_COUNT_MASK; }
    uint32_t refusal = 0;
    for (int64_t t = 0; t < n_tiles; t++)
        refusal |= fq_tile_refusal(info[(size_t)t], final_text || total - prefix[(size_t)t] - (info[(size_t)t] & FQ_COUNT_MASK) > 0u);
    uint32_t lines = total;
    if (final_text && text_bytes > 0) {
        const int64_t p = text_bytes - 1;
        const FqWord v = FQ_LDW(text, p >> 4);
        const uint32_t x[4] = {v.x, v.y, v.z, v.w};
        if (((x[(p & 15) >> 2] >> (8 * (p & 3))) & 0xffu) != 0x0au) lines++;
    }
    // the host entry
    if (refusal & 2u) { R.why = MPB_FQ_WHY_LONE_CR; return R; }
    if (refusal & 1u) { R.why = MPB_FQ_WHY_NON_ASCII; return R; }
    const int64_t cand = (int64_t)lines / 4 < max_records ? (int64_t)lines / 4 : max_records;
    if (cand == 0) return R;
    const int64_t n_start = 4 * cand + 1;
    g_n_start = n_start;
    uint32_t *start = new uint32_t[(size_t)n_start];         // (of the exact size: the sanitizer sees one element past it)
    for (int64_t k = 0; k < n_start; k++) start[k] = 0xffffffffu;
    for (int64_t t = 0; t < n_tiles; t++) model_starts(text, text_bytes, t, prefix[(size_t)t], total, lines, start, n_start);
    // k_fq_rows
    std::vector<int64_t> rows((size_t)cand * 6);
    std::vector<int32_t> kinds((size_t)cand);
    std::vector<mpb_text_row> desc((size_t)cand);
    int64_t first_bad = INT64_MAX, longest = 0;
    bool row_check = false;
    for (int64_t r = 0; r < cand; r++) {
        int32_t kind = 0;
        if (!fq_row(text, text_bytes, start, n_start, r, max_len, &rows[(size_t)r * 6], &kind, &desc[(size_t)r])) { row_check = true; continue; }
        kinds[(size_t)r] = kind;
        if (kind != FQ_REC_OK) { if (r < first_bad) first_bad = r; }
    }
    if (row_check) { R.why = MPB_FQ_WHY_ROW_CHECK; delete[] start; return R; }
    R.n = first_bad == INT64_MAX ? cand : first_bad;
    for (int64_t r = 0; r < R.n; r++) if (desc[(size_t)r].len > longest) longest = desc[(size_t)r].len;
    R.longest = longest;
    R.bad_kind = first_bad == INT64_MAX ? 0 : kinds[(size_t)first_bad];
    R.consumed = R.n > 0 ? (int64_t)FQ_LD_START(start, 4 * R.n) : 0;
    const int64_t keep = R.n + (R.bad_kind ? 1 : 0);
    R.rows.assign(rows.begin(), rows.begin() + keep * 6);
    // k_pack_text's descriptors of the good records: {seq_off, qual_off, min(qual_len, max_len)}
    for (int64_t r = 0; r < R.n; r++) {
        int64_t pl = rows[(size_t)r * 6 + 5];
        if (max_len > 0 && pl > max_len) pl = max_len;
        if (desc[(size_t)r].seq_off != rows[(size_t)r * 6 + 2] || desc[(size_t)r].qual_off != rows[(size_t)r * 6 + 4] || desc[(size_t)r].len != pl) R.why = -1;
    }
    delete[] start;
    return R;
}

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s cases.bin out.bin\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    FILE *o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 2; }
    int32_t cases = 0;
    if (fread(&cases, 4, 1, f) != 1 || cases < 0) { fprintf(stderr, "short header\n"); return 2; }
    long taken = 0, differ = 0, unsupported_taken = 0;
    for (int32_t c = 0; c < cases; c++) {
        int64_t h[2];
        int32_t g[2];
        if (fread(h, 8, 2, f) != 2 || fread(g, 4, 2, f) != 2 || h[0] < 0 || h[0] > (1 << 28) || h[1] < 0) { fprintf(stderr, "bad case header\n"); return 2; }
        const int64_t len = h[0], max_records = h[1], cap = (len + 15) / 16 * 16;
        uint8_t *text = new uint8_t[(size_t)cap + 0];
        if (len && fread(text, 1, (size_t)len, f) != (size_t)len) { fprintf(stderr, "short text\n"); return 2; }
        static const uint8_t pad[3] = {0x0a, 0x0d, 0x80};
        for (int64_t i = len; i < cap; i++) text[i] = pad[i % 3];
        g_text_bytes = len; g_text_cap = cap; g_n_start = 0;
        const Result R = model(text, len, g[0], max_records, g[1]);
        // the yardstick (one row more than the records it can hold: the offender's)
        int64_t host_cap = len / 4 + 2;
        if (max_records + 1 < host_cap) host_cap = max_records + 1;
        std::vector<int64_t> hidx((size_t)host_cap * MIO_IDX_COLS, -1);
        int64_t hcons = 0;
        int32_t hbad = 0;
        const int64_t hn = mio_fastq_index((const char *)text, len, g[0], max_records, hidx.data(), &hcons, &hbad);
        if (R.why == 0) {
            taken++;
            if (hn == MIO_E_UNSUPPORTED) unsupported_taken++;
            bool same = hn == R.n && hcons == R.consumed && hbad == R.bad_kind;
            if (same && !R.rows.empty()) same = memcmp(R.rows.data(), hidx.data(), R.rows.size() * 8) == 0;
            if (!same) {
                differ++;
                fprintf(stderr, "case %d: model n %lld consumed %lld bad %d, host n %lld consumed %lld bad %d\n", c, (long long)R.n,
                        (long long)R.consumed, R.bad_kind, (long long)hn, (long long)hcons, hbad);
            }
        } else if (R.why < 0) {
            differ++;
            fprintf(stderr, "case %d: a descriptor differs from its row\n", c);
        }
        const int32_t w4[2] = {R.why, R.bad_kind};
        const int64_t w8[3] = {R.n, R.consumed, R.longest};
        const int32_t t4[2] = {(int32_t)(hn < 0 ? hn : 0), 0};
        if (fwrite(w4, 4, 2, o) != 2 || fwrite(w8, 8, 3, o) != 3 || fwrite(t4, 4, 2, o) != 2) { fprintf(stderr, "short write\n"); return 2; }
        delete[] text;
    }
    fclose(f);
    fclose(o);
    printf("%d texts, %ld taken, %ld loads or stores out of bounds, %ld differ from mio_fastq_index, %ld unsupported texts taken\n",
           cases, taken, g_oob, differ, unsupported_taken);
    return g_oob ? 3 : (differ || unsupported_taken) ? 4 : 0;
}
