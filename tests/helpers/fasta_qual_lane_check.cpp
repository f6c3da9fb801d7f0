// fasta_qual_lane_check.cpp -- the fasta+qual record stage's lane code (moira_amd/csrc/mpb_fasta_qual_lane.inc, with the line
// kernels' mpb_index_lane.inc behind it) on the host, built with -fsanitize=address,undefined together with csrc/fastio.cpp and
// run as a program (tests/test_fasta_qual_lane_model.py).  The line kernels run over both texts as tests/helpers/
// fastq_index_check.cpp runs them; then 256 lane states run in lockstep as k_fa_count and k_fa_write run them: FA_GROUP lanes per
// record, the group's sums and the exclusive scan of a step made here from the lanes' values; k_fa_scan and the host entry's
// decisions (csrc/mpb_fasta_qual.cpp) are restated.  Each text lies in a heap block of exactly round_up(bytes, 16) bytes whose
// padding holds newlines, carriage returns, digits, blanks and bytes >= 0x80; the line tables lie in blocks of exactly their
// size.  Every load is checked against its block, every store against the record's own slot and against a second store to the
// same byte.  A case that is taken is compared with mio_fasta_qual_index itself: n, both consumed, out_used, out, the rows, and
// the longest packed length; texts the host calls unsupported must not be taken.
//   fasta_qual_lane_check cases.bin  ->  "case NAME: taken n=N fc=F qc=Q used=U longest=L"
//                                      | "case NAME: back why=W which=T bad=R host=RC"   | "case NAME: FAIL what"
// Exit 4 when a case fails.  -DFA_WRONG_NO_VALUE_CAP / -DFA_WRONG_RANK_BY_BYTES: the sensitivity builds.

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "moira_io.h"
#include "moira_pb.h"

struct CheckedText { const uint8_t *p; int64_t bytes, cap; const uint32_t *start; int64_t n_start; };
static CheckedText g_t[2];
static int64_t g_bad_loads, g_bad_stores, g_twice;

struct FqWord { uint32_t x, y, z, w; };
static const CheckedText *text_of(const uint8_t *p) { return p == g_t[0].p ? &g_t[0] : p == g_t[1].p ? &g_t[1] : nullptr; }
static FqWord fq_ldw(const uint8_t *text, int64_t w)
{
    FqWord v = {0, 0, 0, 0};
    const CheckedText *t = text_of(text);
    if (!t || w < 0 || w * 16 >= t->bytes || w * 16 + 16 > t->cap) { g_bad_loads++; return v; }
    memcpy(&v, text + w * 16, 16);
    return v;
}
static uint32_t fq_ldb(const uint8_t *text, int64_t i)
{
    const CheckedText *t = text_of(text);
    if (!t || i < 0 || i >= t->bytes) { g_bad_loads++; return 0; }
    return text[i];
}
static const CheckedText *table_of(const uint32_t *s) { return s == g_t[0].start ? &g_t[0] : s == g_t[1].start ? &g_t[1] : nullptr; }
static uint32_t fq_ld_start(const uint32_t *start, int64_t k)
{
    const CheckedText *t = table_of(start);
    if (!t || k < 0 || k >= t->n_start) { g_bad_loads++; return 0; }
    return start[k];
}
static void fq_st_start(uint32_t *start, int64_t k, uint32_t v)
{
    const CheckedText *t = table_of(start);
    if (!t || k < 0 || k >= t->n_start) { g_bad_stores++; return; }
    start[k] = v;
}

struct CheckedOut { uint8_t *p; uint8_t *seen; int64_t lo, hi; };
static void st8(CheckedOut &o, int64_t pos, uint32_t b)
{
    if (pos < o.lo || pos >= o.hi) { g_bad_stores++; return; }
    if (o.seen[pos]) g_twice++;
    o.seen[pos] = 1;
    o.p[pos] = (uint8_t)b;
}

#define FQ_FN static inline
#define FQ_LDW(text, w) fq_ldw((text), (w))
#define FQ_LDB(text, i) fq_ldb((text), (i))
#define FQ_LD_START(start, k) fq_ld_start((start), (k))
#define FQ_ST_START(start, k, v) fq_st_start((start), (k), (v))
#define FA_FN static inline
#define FA_ST8(o, pos, b) st8((o), (pos), (b))
#include "mpb_fasta_qual_lane.inc"

static_assert(FA_WHY_ROW_CHECK == MPB_FQ_WHY_ROW_CHECK && FA_WHY_NAMES == MPB_FA_WHY_NAMES && FA_WHY_EMPTY == MPB_FA_WHY_EMPTY &&
              FA_WHY_TOKEN == MPB_FA_WHY_TOKEN && FA_WHY_LENGTH == MPB_FA_WHY_LENGTH && MPB_IDX_COLS == MIO_IDX_COLS,
              "the restated constants");

// ---- the line kernels, as tests/helpers/fastq_index_check.cpp runs them ----------------------------------------------------
static uint32_t model_lines(const uint8_t *text, int64_t text_bytes, int64_t tile)
{
    static uint32_t na[FQ_LANES][FQ_TRIPS], cr[FQ_LANES][FQ_TRIPS], count[FQ_LANES];
    static int last[FQ_LANES];
    for (int tid = 0; tid < FQ_LANES; tid++) { count[tid] = 0; last[tid] = 0; }
    for (int t = 0; t < FQ_TRIPS; t++)
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
        static uint32_t nl[FQ_LANES], rank[FQ_LANES];
        uint32_t run = 0;
        for (int tid = 0; tid < FQ_LANES; tid++) {
            const int64_t w = tile * FQ_TILE_WORDS + t * FQ_LANES + tid;
            uint32_t na, cr;
            nl[tid] = 0;
            if (w * FQ_WORD_BYTES < text_bytes) fq_scan_word(text, text_bytes, w, &nl[tid], &na, &cr);
        }
        for (int tid = 0; tid < FQ_LANES; tid++) { rank[tid] = run; run += (uint32_t)__builtin_popcount(nl[tid]); }
        for (int tid = 0; tid < FQ_LANES; tid++)
            if (nl[tid]) fq_store_starts(start, n_start, tile * FQ_TILE_WORDS + t * FQ_LANES + tid, nl[tid], line + rank[tid]);
        line += run;
    }
}

struct Lines { std::vector<uint32_t> info, prefix; uint32_t newlines = 0, refusal = 0, lines = 0; };

static Lines count_lines(const uint8_t *text, int64_t text_bytes, int final_text)
{
    Lines L;
    const int64_t n_tiles = (text_bytes + FQ_TILE - 1) / FQ_TILE;
    L.info.resize((size_t)n_tiles); L.prefix.resize((size_t)n_tiles);
    for (int64_t t = 0; t < n_tiles; t++) L.info[(size_t)t] = model_lines(text, text_bytes, t);
    uint32_t total = 0;
    for (int64_t t = 0; t < n_tiles; t++) { L.prefix[(size_t)t] = total; total += L.info[(size_t)t] & FQ_COUNT_MASK; }
    for (int64_t t = 0; t < n_tiles; t++)
        L.refusal |= fq_tile_refusal(L.info[(size_t)t], final_text || total - L.prefix[(size_t)t] - (L.info[(size_t)t] & FQ_COUNT_MASK) > 0u);
    L.newlines = total; L.lines = total;
    if (final_text && text_bytes > 0 && FQ_LDB(text, text_bytes - 1) != 0x0au) L.lines++;
    return L;
}

// ---- the record stage ------------------------------------------------------------------------------------------------------
struct Result {
    int32_t why = 0, which = 0; int64_t bad = -1, n = 0, fc = 0, qc = 0, used = 0, longest = 0;
    std::vector<int64_t> rows; std::vector<uint8_t> out; std::string fail;
};

struct CaseHead { char name[32]; int64_t flen, qlen, max_records, out_cap; int32_t final_text, max_len; };

static Result model(const CaseHead &h)
{
    Result R;
    const uint8_t *ft = g_t[0].p, *qt = g_t[1].p;
    Lines L[2] = {count_lines(ft, h.flen, h.final_text), count_lines(qt, h.qlen, h.final_text)};
    // the host entry's decisions
    for (int t = 0; t < 2; t++) {
        if (L[t].refusal & 2u) { R.why = MPB_FQ_WHY_LONE_CR; R.which = t; return R; }
        if (L[t].refusal & 1u) { R.why = MPB_FQ_WHY_NON_ASCII; R.which = t; return R; }
    }
    int64_t cand = h.max_records;
    for (int t = 0; t < 2; t++) if ((int64_t)L[t].lines / 2 < cand) cand = (int64_t)L[t].lines / 2;
    if (h.final_text && cand < h.max_records && (L[0].lines > 2 * cand || L[1].lines > 2 * cand)) {
        R.why = MPB_FA_WHY_TRUNCATED; R.which = L[0].lines > 2 * cand ? 0 : 1;
        return R;
    }
    if (cand == 0) return R;
    const int64_t n_start = 2 * cand + 1;
    uint32_t *start[2];
    for (int t = 0; t < 2; t++) {
        start[t] = new uint32_t[(size_t)n_start];            // (of the exact size: the sanitizer sees one element past it)
        for (int64_t k = 0; k < n_start; k++) start[t][k] = 0xffffffffu;
        g_t[t].start = start[t]; g_t[t].n_start = n_start;
        const int64_t n_tiles = (g_t[t].bytes + FQ_TILE - 1) / FQ_TILE;
        for (int64_t tile = 0; tile < n_tiles; tile++)
            model_starts(g_t[t].p, g_t[t].bytes, tile, L[t].prefix[(size_t)tile], L[t].newlines, L[t].lines, start[t], n_start);
    }
    const int per = FA_LANES / FA_GROUP;
    // k_fa_count: the workgroups one after the other, the lanes of one in lockstep
    std::vector<int64_t> size((size_t)cand, 0), prefix((size_t)cand + 1, 0);
    long long status = INT64_MAX;
    for (int64_t g0 = 0; g0 < cand; g0 += per) {
        static FaRec rec[FA_LANES];
        int why[FA_LANES], which[FA_LANES]; bool bad[FA_LANES]; int64_t seps[FA_LANES];
        for (int t = 0; t < FA_LANES; t++) {
            const int64_t r = g0 + t / FA_GROUP;
            why[t] = 0; which[t] = 0; bad[t] = false; seps[t] = 0;
            if (r >= cand) continue;
            why[t] = fa_record(ft, h.flen, start[0], n_start, qt, h.qlen, start[1], n_start, r, true, &rec[t], &which[t]);
            if (why[t] == 0) seps[t] = fa_count_lane(qt, rec[t], t % FA_GROUP, &bad[t]);
        }
        for (int t = 0; t < FA_LANES; t += FA_GROUP) {
            const int64_t r = g0 + t / FA_GROUP;
            if (r >= cand) continue;
            int w = why[t], wh = which[t];
            if (w == 0) {
                int64_t sum = 0; bool any = false;
                for (int j = 0; j < FA_GROUP; j++) { sum += seps[t + j]; any = any || bad[t + j]; }
                w = fa_verdict(rec[t], any, sum); wh = 1;
            }
            size[(size_t)r] = w == 0 ? fa_slot_bytes(rec[t]) : 0;
            if (w != 0 && fa_key(r, w, wh) < status) status = fa_key(r, w, wh);
        }
    }
    // k_fa_scan
    int64_t n_fit = 0;
    for (int64_t r = 0; r < cand; r++) {
        prefix[(size_t)r + 1] = prefix[(size_t)r] + size[(size_t)r];
        if (prefix[(size_t)r + 1] <= h.out_cap) n_fit++;
    }
    if (status != INT64_MAX) {
        R.why = (int32_t)((status >> 1) & 127); R.which = (int32_t)(status & 1); R.bad = status >> 8;
        delete[] start[0]; delete[] start[1];
        return R;
    }
    const int64_t used = prefix[(size_t)n_fit];
    R.out.assign((size_t)used + 1, 0);
    std::vector<uint8_t> seen((size_t)used + 1, 0);
    R.rows.assign((size_t)n_fit * 6, -1);
    // k_fa_write
    for (int64_t g0 = 0; g0 < n_fit; g0 += per) {
        for (int t0 = 0; t0 < FA_LANES; t0 += FA_GROUP) {
            const int64_t r = g0 + t0 / FA_GROUP;
            if (r >= n_fit) continue;
            FaRec rec[FA_GROUP];
            int which;
            const int64_t at = prefix[(size_t)r];
            CheckedOut o{R.out.data(), seen.data(), at, prefix[(size_t)r + 1]};
            for (int j = 0; j < FA_GROUP; j++) {
                if (fa_record(ft, h.flen, start[0], n_start, qt, h.qlen, start[1], n_start, r, false, &rec[j], &which) != 0) R.fail = "k_fa_write refuses a record k_fa_count took";
                fa_copy(ft, rec[j].hdr_off, rec[j].hdr_len, j, o, at);
                fa_copy(ft, rec[j].seq_off, rec[j].seq_len, j, o, at + rec[j].hdr_len);
            }
            const int64_t qat = at + rec[0].hdr_len + rec[0].seq_len, w1 = fa_end_word(rec[0]);
            int64_t before = 0;
            for (int64_t w0 = fa_first_word(rec[0]); w0 < w1; w0 += FA_GROUP) {
                FaQ q[FA_GROUP]; int mine[FA_GROUP];
                for (int j = 0; j < FA_GROUP; j++) {
                    mine[j] = 0;
                    if (w0 + j < w1) { fa_qload(qt, rec[j], w0 + j, &q[j]); mine[j] = fa_qseps(q[j]); }
                }
                int excl = 0;
                for (int j = 0; j < FA_GROUP; j++) {
                    if (w0 + j < w1) fa_qstore(q[j], rec[j], before + excl, o, qat);
                    excl += mine[j];
                }
                before += excl;
            }
            mpb_text_row d;
            fa_row_out(rec[0], at, h.max_len, &R.rows[(size_t)r * 6], &d);
            if (d.seq_off != R.rows[(size_t)r * 6 + 2] || d.qual_off != R.rows[(size_t)r * 6 + 4]) R.fail = "a descriptor differs from its row";
            if (d.len > R.longest) R.longest = d.len;
        }
    }
    if (R.fail.empty() && (int64_t)std::count(seen.begin(), seen.begin() + used, 1) != used) R.fail = "a byte of a slot was never stored";
    R.n = n_fit; R.used = used;
    R.fc = n_fit > 0 ? (int64_t)FQ_LD_START(start[0], 2 * n_fit) : 0;
    R.qc = n_fit > 0 ? (int64_t)FQ_LD_START(start[1], 2 * n_fit) : 0;
    delete[] start[0]; delete[] start[1];
    return R;
}

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t n_cases = 0;
    if (fread(&n_cases, 4, 1, f) != 1) return 2;
    int fails = 0, taken = 0, unsupported_taken = 0;
    int64_t all_bad_loads = 0;
    for (int ci = 0; ci < n_cases; ci++) {
        CaseHead h;
        if (fread(&h, sizeof(h), 1, f) != 1 || h.flen < 0 || h.qlen < 0 || h.flen > (1 << 28) || h.qlen > (1 << 28) || h.out_cap < 0) return 2;
        h.name[31] = 0;
        uint8_t *text[2];
        const int64_t len[2] = {h.flen, h.qlen};
        static const uint8_t pad[5] = {0x0a, 0x0d, 0x80, '9', ' '};
        for (int t = 0; t < 2; t++) {
            const int64_t cap = (len[t] + 15) / 16 * 16;
            text[t] = new uint8_t[(size_t)cap + 0];          // exactly the words the kernels may ask for
            if (len[t] && fread(text[t], 1, (size_t)len[t], f) != (size_t)len[t]) return 2;
            for (int64_t i = len[t]; i < cap; i++) text[t][i] = pad[i % 5];
            g_t[t] = CheckedText{text[t], len[t], cap, nullptr, 0};
        }
        g_bad_loads = 0; g_bad_stores = 0; g_twice = 0;
        Result R = model(h);
        // the yardstick
        int64_t rows_cap = h.flen / 2 + 2;
        if (h.max_records < rows_cap) rows_cap = h.max_records;
        std::vector<int64_t> hidx((size_t)(rows_cap + 1) * MIO_IDX_COLS, -1);
        std::vector<char> hout((size_t)h.out_cap + 1, 0);
        int64_t hfc = 0, hqc = 0, hused = 0;
        // (the host function wants non-null texts; an empty one is a block of no bytes here)
        const int64_t hn = mio_fasta_qual_index((const char *)text[0], h.flen, (const char *)text[1], h.qlen, h.final_text, h.max_records,
                                                hout.data(), h.out_cap, hidx.data(), &hfc, &hqc, &hused);
        std::string what = R.fail;
        if (what.empty() && g_bad_loads) what = "loads out of bounds";
        if (what.empty() && g_bad_stores) what = "stores outside the record's slot or a table";
        if (what.empty() && g_twice) what = "a byte stored twice";
        if (what.empty() && R.why == 0) {
            taken++;
            if (hn < 0) { unsupported_taken++; what = "taken, but the host says " + std::to_string((long long)hn); }
            else if (hn != R.n || hfc != R.fc || hqc != R.qc || hused != R.used)
                what = "n / consumed / used " + std::to_string((long long)R.n) + " " + std::to_string((long long)R.fc) + " " +
                       std::to_string((long long)R.qc) + " " + std::to_string((long long)R.used) + ", the host's " + std::to_string((long long)hn) + " " +
                       std::to_string((long long)hfc) + " " + std::to_string((long long)hqc) + " " + std::to_string((long long)hused);
            else if (R.used && memcmp(R.out.data(), hout.data(), (size_t)R.used) != 0) {
                int64_t at = 0;
                while (R.out[(size_t)at] == (uint8_t)hout[(size_t)at]) at++;
                what = "byte " + std::to_string((long long)at) + " of out differs from the host's: " + std::to_string((int)R.out[(size_t)at]) +
                       " for " + std::to_string((int)(uint8_t)hout[(size_t)at]);
            }
            else if (R.n && memcmp(R.rows.data(), hidx.data(), (size_t)R.n * 48) != 0) what = "a row differs from the host's";
            else {
                int64_t longest = 0;
                for (int64_t r = 0; r < hn; r++) {
                    int64_t pl = hidx[(size_t)r * 6 + 3];
                    if (h.max_len > 0 && pl > h.max_len) pl = h.max_len;
                    if (pl > longest) longest = pl;
                }
                if (longest != R.longest) what = "the longest packed length differs";
            }
        }
        all_bad_loads += g_bad_loads;
        if (!what.empty()) { printf("case %s: FAIL %s\n", h.name, what.c_str()); fails++; }
        else if (R.why == 0)
            printf("case %s: taken n=%lld fc=%lld qc=%lld used=%lld longest=%lld\n", h.name, (long long)R.n, (long long)R.fc, (long long)R.qc,
                   (long long)R.used, (long long)R.longest);
        else printf("case %s: back why=%d which=%d bad=%lld host=%lld\n", h.name, R.why, R.which, (long long)R.bad, (long long)(hn < 0 ? hn : 0));
        delete[] text[0]; delete[] text[1];
    }
    fclose(f);
    printf("%d cases, %d taken, %lld loads out of bounds, %d unsupported texts taken, %d fail\n", n_cases, taken, (long long)all_bad_loads,
           unsupported_taken, fails);
    return fails ? 4 : 0;
}
