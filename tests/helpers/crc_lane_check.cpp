// Host twin of the device CRC-32 (moira_amd/csrc/mpb_crc_kernels.hip): the per-lane code of moira_amd/csrc/mpb_crc_lane.inc
// compiled for the host and run as k_bgzf_crc32 runs it -- the 64 lane states of a wave take every step in lockstep, then the
// wave's xor.  A text lies in a heap block of exactly its size; every load goes through an accessor that checks it against the
// LANE'S SLICE (and a word load against its alignment): one outside is counted, not made, and fails the run (exit status 3).
// tests/test_crc_lane_model.py builds this program with the address and undefined-behaviour sanitizers together with
// csrc/mpb_hostonly.cpp; every range is compared here with bgzf_crc32 and with the zlib.crc32 value the test passes in, the four
// tables with RFC 1952's bit loop, and the 64 slice factors with x^(8192 j) by square-and-multiply.
//
// Input (argv[1]): little-endian  int32 texts;  per text  int64 bytes, int32 ranges, int32 pad, the text,
//                  then per range  int64 off, int32 len, uint32 zlib_crc (ignored for a range outside the text).
// Output (argv[2]): per range  uint32 crc, uint32 bad.
// Prints "<r> ranges, <b> refused, <o> loads out of bounds, <d> differ from bgzf_crc32, <z> differ from zlib.crc32, <t> table or
// factor words differ".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mpb_hostonly.h"

static int64_t g_lo = 0, g_hi = 0;               // the slice of the lane that is taking its step
static long g_oob = 0;

struct CrcWord { uint32_t x, y, z, w; };
#define CRC_FN static inline
#define CRC_CONST static const
static inline CrcWord crc_ldw(const uint8_t *text, int64_t p)
{
    CrcWord v = {0, 0, 0, 0};
    if ((p & 15) != 0 || p < g_lo || p + 16 > g_hi) { g_oob++; return v; }
    memcpy(&v, text + p, 16);
    return v;
}
static inline uint32_t crc_ldb(const uint8_t *text, int64_t p)
{
    if (p < g_lo || p >= g_hi) { g_oob++; return 0; }
    return text[p];
}
static inline uint32_t crc_tab(const uint32_t *tab, int k, uint32_t i)
{
    if (k < 0 || k > 3 || i > 255u) { g_oob++; return 0; }
    return tab[k * 256 + i];
}
#define CRC_LDW(text, p) crc_ldw((text), (p))
#define CRC_LDB(text, p) crc_ldb((text), (p))
#define CRC_TAB(tab, k, i) crc_tab((tab), (k), (i))
#include "mpb_crc_lane.inc"

// one range as one wave: false when the kernel would refuse it
static bool model(const uint8_t *text, int64_t text_bytes, const uint32_t *tab, int64_t off, int64_t len, uint32_t *crc)
{
    *crc = 0;
    if (!crc_range_ok(off, len, text_bytes)) return false;
    CrcLane L[CRC_LANES];
    int64_t lo[CRC_LANES], hi[CRC_LANES];
    for (int j = 0; j < CRC_LANES; j++) {
        crc_lane_begin(off, len, j, &L[j]);
        lo[j] = L[j].p; hi[j] = L[j].end;
        if (lo[j] < off || hi[j] > off + len || lo[j] > hi[j]) g_oob++;     // a slice outside its range
    }
    for (bool any = true; any;) {                            // (a trip is one step of every lane)
        any = false;
        for (int j = 0; j < CRC_LANES; j++) {
            g_lo = lo[j]; g_hi = hi[j];
            if (crc_lane_step(text, tab, &L[j])) any = true;
        }
    }
    uint32_t v = 0;
    for (int j = 0; j < CRC_LANES; j++) v ^= crc_lane_end(&L[j], j);
    *crc = v ^ 0xffffffffu;
    return true;
}

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s cases.bin out.bin\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    FILE *o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 2; }
    // the tables as the workgroup fills them, against RFC 1952's loop; the factors against square-and-multiply
    long tab_differ = 0;
    std::vector<uint32_t> tab(4 * 256);
    for (uint32_t i = 0; i < 256; i++) {
        uint32_t e[4];
        crc_table_entry(i, e);
        for (int k = 0; k < 4; k++) tab[(size_t)k * 256 + i] = e[k];
    }
    for (uint32_t i = 0; i < 256; i++) {
        uint32_t c = i;
        for (int k = 0; k < 4; k++) {
            for (int s = 0; s < 8; s++) c = (c & 1) ? CRC_POLY ^ (c >> 1) : c >> 1;
            if (tab[(size_t)k * 256 + i] != c) tab_differ++;
        }
    }
    {
        uint32_t step = 0x80000000u >> 1;                    // x^1, squared 13 times: x^8192
        for (int s = 0; s < 13; s++) step = crc_mulmod(step, step);
        uint32_t want = 0x80000000u;                         // x^0
        for (int j = 0; j < CRC_LANES; j++) { if (crc_slice_factor[j] != want) tab_differ++; want = crc_mulmod(want, step); }
    }
    int32_t texts = 0;
    if (fread(&texts, 4, 1, f) != 1 || texts < 0) { fprintf(stderr, "short header\n"); return 2; }
    long ranges = 0, refused = 0, differ = 0, differ_zlib = 0;
    for (int32_t t = 0; t < texts; t++) {
        int64_t bytes = 0;
        int32_t g[2];
        if (fread(&bytes, 8, 1, f) != 1 || fread(g, 4, 2, f) != 2 || bytes < 0 || bytes > (1 << 28) || g[0] < 0) { fprintf(stderr, "bad text header\n"); return 2; }
        uint8_t *text = new uint8_t[(size_t)bytes];          // (of the exact size: the sanitizer sees one byte past it)
        if (bytes && fread(text, 1, (size_t)bytes, f) != (size_t)bytes) { fprintf(stderr, "short text\n"); return 2; }
        for (int32_t r = 0; r < g[0]; r++) {
            int64_t off = 0;
            int32_t len = 0;
            uint32_t zcrc = 0;
            if (fread(&off, 8, 1, f) != 1 || fread(&len, 4, 1, f) != 1 || fread(&zcrc, 4, 1, f) != 1) { fprintf(stderr, "short range\n"); return 2; }
            uint32_t w[2] = {0, 0};
            ranges++;
            if (model(text, bytes, tab.data(), off, len, &w[0])) {
                if (w[0] != bgzf_crc32(text + off, (size_t)len)) differ++;
                if (w[0] != zcrc) {
                    differ_zlib++;
                    if (differ_zlib <= 5) fprintf(stderr, "text %d range %d (off %lld, len %d): model %08x, zlib %08x\n", t, r, (long long)off, len, w[0], zcrc);
                }
            } else {
                refused++;
                w[1] = CRC_BAD_RANGE;
            }
            if (fwrite(w, 4, 2, o) != 2) { fprintf(stderr, "short write\n"); return 2; }
        }
        delete[] text;
    }
    fclose(f);
    fclose(o);
    printf("%ld ranges, %ld refused, %ld loads out of bounds, %ld differ from bgzf_crc32, %ld differ from zlib.crc32, %ld table or factor words differ\n",
           ranges, refused, g_oob, differ, differ_zlib, tab_differ);
    return g_oob ? 3 : (differ || differ_zlib || tab_differ) ? 4 : 0;
}
