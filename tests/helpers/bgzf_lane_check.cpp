// bgzf_lane_check.cpp -- the per-lane code of k_bgzf_deflate (moira_amd/csrc/mpb_bgzf_lane.inc) on the host: a whole member goes
// through 256 lane states in the kernel's order (all look-ups of a step, then all insertions with the largest position winning,
// then the verified matches, the greedy walk, the tokens; the plan; the header and the tokens at their scanned bit offsets), with
// every load of the text checked against the member's bounds, and the Huffman length builder runs alone on given histograms.
// Built with -fsanitize=address,undefined by tests/test_bgzf_lane_model.py and run as a program.
// Three compile-time switches, for tests/test_bgzf_model_streams.py alone (none set: the kernel's order and the format below):
//   -DBZ_CHECK_INSERT_FIRST    a step's insertions precede its look-ups (what a missing barrier could give)
//   -DBZ_CHECK_SMALLEST_WINS   of a step's positions in one bucket the smallest wins (what another order of plain stores could give)
//   -DBZ_CHECK_HISTOGRAMS      after a member's stream: its 286 literal/length and 30 distance counts as uint32
//
//   in : int32 cases, then per case  int32 kind, int32 n,  kind 0: n text bytes;  kind 1: int32 limit, n uint32 counts
//   out: per case  kind 0: int32 btype, bytes, literals, matches, matched, loads out of bounds, hlit, hdist; 288 + 32 + 19 code
//                          lengths of the dynamic trees as built (before the choice); the stream
//                  kind 1: n code lengths
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#define MPB_BGZF_DATA 0xff00

static int g_n = 0;
static long g_oob = 0;
static inline uint8_t ld8_checked(const uint8_t *text, int i)
{
    if (i < 0 || i >= g_n) { g_oob++; return 0; }
    return text[i];
}
static inline uint64_t ld64_checked(const uint8_t *text, int i, int n)
{
    uint64_t v = 0;
    for (int k = 0; k < 8 && i + k < n; k++) v |= (uint64_t)ld8_checked(text, i + k) << (8 * k);
    return v;
}
#define BZ_FN static inline
#define BZ_LD8(text, i) ld8_checked((text), (i))
#define BZ_LD64(text, i, n) ld64_checked((text), (i), (n))
#define BZ_OR32(ptr, value) (*(ptr) |= (value))
#include "mpb_bgzf_lane.inc"

static void put32(std::vector<uint8_t> &o, int32_t v) { uint8_t b[4]; memcpy(b, &v, 4); o.insert(o.end(), b, b + 4); }

// the insertions of one step: every bucket ends with the largest position + 1 of the step that fell into it (the kernel's atomic
// max; positions grow from step to step, so a bucket never holds more than a step's largest)
static void insert_step(std::vector<uint32_t> &hash, const uint32_t *ha, const uint32_t *hb, int base)
{
#ifdef BZ_CHECK_SMALLEST_WINS
    for (int t = BZ_STEP - 1; t >= 0; t--) {                 // plain stores, the smallest position last
        if (ha[t] != BZ_NO_HASH) hash[ha[t]] = (uint32_t)(base + t) + 1u;
        if (hb[t] != BZ_NO_HASH) hash[hb[t]] = (uint32_t)(base + t) + 1u;
    }
#else
    for (int t = 0; t < BZ_STEP; t++) {
        const uint32_t v = (uint32_t)(base + t) + 1u;
        if (ha[t] != BZ_NO_HASH && hash[ha[t]] < v) hash[ha[t]] = v;
        if (hb[t] != BZ_NO_HASH && hash[hb[t]] < v) hash[hb[t]] = v;
    }
#endif
}

static bool member(const uint8_t *text, int n, std::vector<uint8_t> &out)
{
    if (n < 1 || n > MPB_BGZF_DATA) return false;
    g_n = n; g_oob = 0;
    std::vector<uint32_t> hash(BZ_HASH_SIZE, 0), tok((size_t)n, 0);
    static BzCoder cd;
    memset(&cd, 0, sizeof(cd));
    int cur = 0;
    for (int base = 0; base < n; base += BZ_STEP) {
        uint32_t ha[BZ_STEP], hb[BZ_STEP], ca[BZ_STEP], cb[BZ_STEP];
        uint16_t slen[BZ_STEP]; uint8_t sflag[BZ_STEP]; int len[BZ_STEP], dist[BZ_STEP];
        for (int t = 0; t < BZ_STEP; t++) {
            const int p = base + t;
            ha[t] = p < n ? bz_hash_a(text, n, p) : BZ_NO_HASH;
            hb[t] = p < n ? bz_hash_b(text, n, p) : BZ_NO_HASH;
        }
#ifdef BZ_CHECK_INSERT_FIRST
        insert_step(hash, ha, hb, base);
#endif
        for (int t = 0; t < BZ_STEP; t++) {
            ca[t] = ha[t] != BZ_NO_HASH ? hash[ha[t]] : 0;
            cb[t] = hb[t] != BZ_NO_HASH ? hash[hb[t]] : 0;
        }
#ifndef BZ_CHECK_INSERT_FIRST
        insert_step(hash, ha, hb, base);
#endif
        for (int t = 0; t < BZ_STEP; t++) {
            const int p = base + t;
            len[t] = 0; dist[t] = 0;
            if (p < n) bz_find(text, n, p, ca[t], cb[t], &len[t], &dist[t]);
            slen[t] = (uint16_t)len[t]; sflag[t] = 0;
        }
        cur = bz_walk_step(slen, sflag, base, n - base < BZ_STEP ? n - base : BZ_STEP, cur);
        for (int t = 0; t < BZ_STEP; t++) {
            const int p = base + t;
            if (p >= n || !sflag[t]) continue;
            if (len[t]) {
                int ls, le, lv, ds, de, dv;
                bz_len_code(len[t], &ls, &le, &lv);
                bz_dist_code(dist[t], &ds, &de, &dv);
                tok[(size_t)p] = bz_tok_match(len[t], dist[t]);
                cd.ll_freq[ls]++; cd.d_freq[ds]++; cd.n_match++; cd.matched += (uint32_t)len[t];
            } else {
                tok[(size_t)p] = bz_tok_literal(BZ_LD8(text, p));
                cd.ll_freq[BZ_LD8(text, p)]++; cd.n_lit++;
            }
        }
    }
    // the dynamic trees as built, for the Kraft sums (bz_plan_block overwrites them when it chooses the fixed code)
    uint8_t ll[BZ_NLL] = {0}, dl[BZ_ND] = {0};
    cd.ll_freq[BZ_EOB] = 1;
#ifdef BZ_CHECK_HISTOGRAMS
    std::vector<uint32_t> hist(cd.ll_freq, cd.ll_freq + 286);
    hist.insert(hist.end(), cd.d_freq, cd.d_freq + 30);
#endif
    bz_build_lengths(cd.ll_freq, 286, 15, ll, &cd.tree);
    bz_build_lengths(cd.d_freq, 30, 15, dl, &cd.tree);
    bz_plan_block(&cd, n);
    std::vector<uint8_t> stream;
    if (cd.btype == BZ_STORED) {
        stream.resize((size_t)n + 5);
        stream[0] = 1; stream[1] = (uint8_t)(n & 0xff); stream[2] = (uint8_t)(n >> 8);
        stream[3] = (uint8_t)(~n & 0xff); stream[4] = (uint8_t)((~n >> 8) & 0xff);
        for (int i = 0; i < n; i++) stream[5 + (size_t)i] = BZ_LD8(text, i);
    } else {
        const size_t nw = (cd.total_bits + 31u) >> 5;
        std::vector<uint32_t> words(nw + 1, 0);
        bz_write_header(&cd, words.data());
        uint32_t pos = cd.hdr_bits;
        for (int p = 0; p < n; p++) {
            const uint32_t w = (uint32_t)bz_token_bits(&cd, tok[(size_t)p]);
            if (pos + w > cd.total_bits) { fprintf(stderr, "token at %d runs past the planned %u bits\n", p, cd.total_bits); return false; }
            bz_emit_token(&cd, words.data(), pos, tok[(size_t)p]);
            pos += w;
        }
        bz_put(words.data(), pos, cd.ll_code[BZ_EOB], cd.ll_len[BZ_EOB]);
        pos += cd.ll_len[BZ_EOB];
        if (pos != cd.total_bits) { fprintf(stderr, "planned %u bits, wrote %u\n", cd.total_bits, pos); return false; }
        stream.resize((cd.total_bits + 7u) >> 3);
        for (size_t i = 0; i < stream.size(); i++) stream[i] = (uint8_t)(words[i >> 2] >> (8 * (i & 3)));
    }
    if (cd.n_lit + cd.matched != (uint32_t)n) { fprintf(stderr, "tokens cover %u of %d bytes\n", cd.n_lit + cd.matched, n); return false; }
    put32(out, cd.btype); put32(out, (int32_t)stream.size()); put32(out, (int32_t)cd.n_lit); put32(out, (int32_t)cd.n_match);
    put32(out, (int32_t)cd.matched); put32(out, (int32_t)g_oob); put32(out, cd.hlit); put32(out, cd.hdist);
    out.insert(out.end(), ll, ll + BZ_NLL); out.insert(out.end(), dl, dl + BZ_ND); out.insert(out.end(), cd.cl_len, cd.cl_len + BZ_NCL);
    out.insert(out.end(), stream.begin(), stream.end());
#ifdef BZ_CHECK_HISTOGRAMS
    for (uint32_t f : hist) put32(out, (int32_t)f);
#endif
    return true;
}

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s cases.bin out.bin\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<uint8_t> in;
    uint8_t buf[65536];
    size_t got;
    while ((got = fread(buf, 1, sizeof(buf), f)) > 0) in.insert(in.end(), buf, buf + got);
    fclose(f);
    size_t pos = 0;
    auto get32 = [&](int32_t *v) { if (pos + 4 > in.size()) return false; memcpy(v, &in[pos], 4); pos += 4; return true; };
    int32_t cases = 0;
    if (!get32(&cases)) return 2;
    std::vector<uint8_t> out;
    long oob = 0;
    for (int32_t k = 0; k < cases; k++) {
        int32_t kind = 0, n = 0;
        if (!get32(&kind) || !get32(&n) || n < 0) return 2;
        if (kind == 0) {
            if (pos + (size_t)n > in.size()) return 2;
            std::vector<uint8_t> text(in.begin() + (long)pos, in.begin() + (long)pos + n);      // its own allocation: the sanitizer sees its end
            pos += (size_t)n;
            if (!member(text.data(), n, out)) { fprintf(stderr, "case %d failed\n", k); return 1; }
            oob += g_oob;
        } else {
            int32_t limit = 0;
            if (!get32(&limit) || n > BZ_NLL || pos + 4 * (size_t)n > in.size()) return 2;
            std::vector<uint32_t> freq((size_t)n);
            if (n) memcpy(freq.data(), &in[pos], 4 * (size_t)n);
            pos += 4 * (size_t)n;
            std::vector<uint8_t> len((size_t)n + 2, 0);
            static BzTree tree;
            bz_build_lengths(freq.data(), n, limit, len.data(), &tree);
            out.insert(out.end(), len.begin(), len.begin() + n);
        }
    }
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    fwrite(out.data(), 1, out.size(), f);
    fclose(f);
    printf("%d cases, %ld loads out of bounds\n", cases, oob);
    return 0;
}
