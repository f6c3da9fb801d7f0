// inflate_lane_check.cpp -- the lane code of k_bgzf_inflate (moira_amd/csrc/mpb_inflate_lane.inc) on the host: every raw-deflate
// stream goes through bi_member with 64 lane states in lockstep (BI_EACH runs each step for all 64 lanes in turn; what the lanes
// share -- window, ring, tables -- are allocations of their exact sizes, so the sanitizer sees their ends), with every load of the
// compressed bytes and every store of the text checked against the stream's and the text's bounds.  The 64 states must end equal.
// Built with -fsanitize=address,undefined by tests/test_inflate_lane_model.py and run as a program.
//
//   in : int32 cases, then per case  int32 stream_len, out_len, lead (bytes in front of the stream), shift (bytes in front of the
//        text), then the stream
//   out: per case  int32 why, iterations, cap (8 * stream_len + 8), loads and stores out of bounds, lane states that differ,
//        stored, fixed, dynamic blocks, literals, matches, matched bytes, longest code, text bytes that follow; the text
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

static int64_t g_lo = 0, g_hi = 0, g_text_lo = 0, g_text_hi = 0;
static long g_oob = 0;
static inline void ld_in16(const uint8_t *in, int64_t q, uint32_t *w)
{
    if (q < g_lo || q + 16 > g_hi || (q & 15)) { g_oob++; w[0] = w[1] = w[2] = w[3] = 0; return; }
    memcpy(w, in + q, 16);
}
static inline uint8_t ld_in8(const uint8_t *in, int64_t q)
{
    if (q < g_lo || q >= g_hi) { g_oob++; return 0; }
    return in[q];
}
static inline void st_out16(uint8_t *text, int64_t q, const uint32_t *w)
{
    if (q < g_text_lo || q + 16 > g_text_hi || (q & 15)) { g_oob++; return; }
    memcpy(text + q, w, 16);
}
static inline void st_out8(uint8_t *text, int64_t q, uint8_t b)
{
    if (q < g_text_lo || q >= g_text_hi) { g_oob++; return; }
    text[q] = b;
}
#define BI_FN static inline
#define BI_LD_IN16(in, q, w) ld_in16((in), (q), (w))
#define BI_LD_IN8(in, q) ld_in8((in), (q))
#define BI_ST_OUT16(text, q, w) st_out16((text), (q), (w))
#define BI_ST_OUT8(text, q, b) st_out8((text), (q), (b))
#define BI_ATOMIC_INC(ptr) (*(ptr) += 1u)
#define BI_SYNC() do { } while (0)
#define BI_STATES 64
#define BI_EACH(lane, lane0) for (int lane = 0; lane < 64; lane++)
#define BI_I(lane) (lane)
#include "mpb_inflate_lane.inc"

static void put32(std::vector<uint8_t> &o, int32_t v) { uint8_t b[4]; memcpy(b, &v, 4); o.insert(o.end(), b, b + 4); }

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
    long oob = 0, differ = 0, capped = 0;
    for (int32_t k = 0; k < cases; k++) {
        int32_t stream_len = 0, out_len = 0, lead = 0, shift = 0;
        if (!get32(&stream_len) || !get32(&out_len) || !get32(&lead) || !get32(&shift)) return 2;
        if (stream_len < 0 || stream_len > 65536 || out_len < 0 || out_len > BI_WINDOW || lead < 0 || shift < 0) return 2;
        if (pos + (size_t)stream_len > in.size()) return 2;
        // allocations of their own, of the exact sizes
        std::vector<uint8_t> piece((size_t)lead + (size_t)stream_len, 0xa5);
        if (stream_len) memcpy(piece.data() + lead, &in[pos], (size_t)stream_len);
        pos += (size_t)stream_len;
        std::vector<uint32_t> window(BI_WINDOW / 4, 0xdeadbeefu);
        std::vector<uint8_t> text((size_t)shift + (size_t)out_len, 0x5a);
        std::vector<BiShared> sh(1);
        std::vector<BiLane> L(BI_STATES);
        g_lo = lead; g_hi = (int64_t)lead + stream_len; g_text_lo = shift; g_text_hi = (int64_t)shift + out_len; g_oob = 0;
        uint32_t iterations = 0;
        const uint32_t why = bi_member(piece.data(), lead, (uint32_t)stream_len, (uint32_t)out_len, (uint8_t *)window.data(), sh.data(),
                                       L.data(), 0, &iterations);
        long d = 0;
        for (int lane = 1; lane < BI_STATES; lane++) d += memcmp(&L[0], &L[(size_t)lane], sizeof(BiLane)) != 0;
        if (why == BI_OK)
            for (int lane = 0; lane < BI_LANES; lane++) bi_store_window(window.data(), text.data(), shift, (uint32_t)out_len, lane);
        const uint32_t cap = 8u * (uint32_t)stream_len + 8u;
        put32(out, (int32_t)why); put32(out, (int32_t)iterations); put32(out, (int32_t)cap); put32(out, (int32_t)g_oob); put32(out, (int32_t)d);
        put32(out, (int32_t)L[0].stored_blocks); put32(out, (int32_t)L[0].fixed_blocks); put32(out, (int32_t)L[0].dynamic_blocks);
        put32(out, (int32_t)L[0].literals); put32(out, (int32_t)L[0].matches); put32(out, (int32_t)L[0].matched_bytes);
        put32(out, (int32_t)L[0].longest_code);
        const int32_t nt = why == BI_OK ? out_len : 0;
        put32(out, nt);
        out.insert(out.end(), text.begin() + shift, text.begin() + shift + nt);
        for (int32_t i = 0; i < shift; i++) if (text[(size_t)i] != 0x5a) g_oob++;      // nothing in front of the text was touched
        oob += g_oob; differ += d; capped += iterations > cap;
    }
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    fwrite(out.data(), 1, out.size(), f);
    fclose(f);
    printf("%d cases, %ld loads out of bounds, %ld lane states differ, %ld over the cap\n", cases, oob, differ, capped);
    return 0;
}
