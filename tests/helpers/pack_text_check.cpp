// Host twin of k_pack_text's per-chunk code (tests/test_text_rows.py cuts decode4_bytes .. decode16 and pack16 .. fetch16 out of
// moira_amd/csrc/mpb_kernels.hip into pack_text_funcs.h): every row is packed chunk by chunk as the kernel's lanes do and compared
// with mio_pack (csrc/fastio.cpp, linked in) -- the whole matrix, the lengths, the flags and the first bad record.  The
// 16-byte loads go through a checked gload16: a load outside [text, text + round_up(text_bytes, 16)) or off alignment fails the
// run, and the capacity bytes past text_bytes are filled with 0xFF and with 'N' in turn.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "moira_io.h"

struct uint4 { uint32_t x, y, z, w; };
static inline uint4 make_uint4(uint32_t x, uint32_t y, uint32_t z, uint32_t w) { return uint4{x, y, z, w}; }
#define __device__
#define __forceinline__ inline
#define __restrict__
using std::min;
static inline uint32_t __builtin_amdgcn_alignbyte(uint32_t hi, uint32_t lo, uint32_t sh)
{
    return (uint32_t)(((((uint64_t)hi) << 32) | lo) >> (8 * (sh & 3)));
}
static const uint8_t *g_lo, *g_hi;
static long g_oob = 0;
static inline uint4 gload16(const uint8_t *p)
{
    uint4 v{0, 0, 0, 0};
    if (p < g_lo || p + 16 > g_hi || ((uintptr_t)(p - g_lo) & 15)) { g_oob++; return v; }
    memcpy(&v, p, 16);
    return v;
}
#define MPB_PT_BELOW 1u
#define MPB_PT_ABOVE 2u
#define MPB_PT_UPPER 4u
#include "pack_text_funcs.h"

struct Row { int64_t seq_off, qual_off; int32_t len; };

template <bool LOWER>
static void pack_rows(const uint8_t *text, const std::vector<Row> &rows, int offset, int64_t stride, uint8_t *out, int32_t *len_out,
                      uint8_t *flags, int64_t status[2])
{
    const int cpr = (int)(stride >> 4);
    for (size_t k = 0; k < rows.size(); k++) {
        const Row &r = rows[k];
        uint32_t st = 0;
        for (int c = 0; c < cpr; c++) {
            const int nv = r.len - 16 * c;
            uint4 o = make_uint4(0u, 0u, 0u, 0u);
            if (nv > 0) {
                const int m = min(nv, 16);
                const uint4 ql = fetch16(text, r.qual_off + 16 * c, m);
                const uint4 sq = fetch16(text, r.seq_off + 16 * c, m);
                o = pack16<LOWER>(sq, ql, nv, offset, st);
            }
            memcpy(out + (int64_t)k * stride + 16 * c, &o, 16);
        }
        len_out[k] = r.len;
        flags[k] = (st & MPB_PT_UPPER) ? 1 : 0;
        if ((st & MPB_PT_BELOW) && (int64_t)k < status[0]) status[0] = (int64_t)k;
        if ((st & MPB_PT_ABOVE) && (int64_t)k < status[1]) status[1] = (int64_t)k;
    }
}

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 32);
}

int main()
{
    long mismatches = 0, cases = 0;
    for (int trial = 0; trial < 400; trial++) {
        const int offset = trial % 5 == 4 ? 0 : (trial % 2 ? 64 : 33);
        const int lower = (trial / 2) % 2;
        const int n = 1 + (int)(rnd() % 40);
        const bool plant_bad = trial % 7 == 3;
        // records at arbitrary offsets, sequence and quality lines independently placed; the last one ends at the last byte
        std::vector<uint8_t> text;
        std::vector<int64_t> idx((size_t)n * MIO_IDX_COLS, 0);
        int longest = 1;
        for (int i = 0; i < n; i++) {
            static const int lens[] = {0, 1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 300};
            const int len = lens[rnd() % 18];
            longest = std::max(longest, len);
            for (uint32_t g = rnd() % 19; g > 0; g--) text.push_back((uint8_t)(rnd() % 4 == 0 ? 'N' : 0xff));
            idx[(size_t)i * MIO_IDX_COLS + MIO_SEQ_OFF] = (int64_t)text.size();
            idx[(size_t)i * MIO_IDX_COLS + MIO_SEQ_LEN] = len;
            const bool all_n = rnd() % 23 == 0;
            for (int b = 0; b < len; b++) {
                const uint32_t r = rnd() % 40;
                text.push_back(all_n ? 'N' : r == 0 ? 'N' : r == 1 ? 'n' : r == 2 ? 'M' : r == 3 ? 'O' : "ACGT"[r & 3]);
            }
            for (uint32_t g = rnd() % 19; g > 0; g--) text.push_back((uint8_t)(rnd() % 4 == 0 ? 'n' : 0x00));
            idx[(size_t)i * MIO_IDX_COLS + MIO_QUAL_OFF] = (int64_t)text.size();
            idx[(size_t)i * MIO_IDX_COLS + MIO_QUAL_LEN] = len;
            for (int b = 0; b < len; b++) {
                uint32_t q = rnd() % 42;
                if (rnd() % 9 == 0) q = 0;
                uint32_t ch = (uint32_t)offset + q;
                if (plant_bad && rnd() % 200 == 0) ch = offset > 0 ? (uint32_t)offset - 1 - rnd() % (uint32_t)offset : 255u;
                if (offset == 0 && rnd() % 97 == 0) ch = 254;
                text.push_back((uint8_t)ch);
            }
        }
        const int64_t text_bytes = (int64_t)text.size();
        const int64_t cap = (text_bytes + 15) / 16 * 16;
        const int max_len = trial % 3 == 0 ? 0 : (int)(1 + rnd() % 310);
        int packed_longest = max_len > 0 ? std::min(longest, max_len) : longest;
        const int64_t strides[3] = {(packed_longest + 127) / 128 * 128, (packed_longest + 15) / 16 * 16, (packed_longest + 15) / 16 * 16 + 48};
        const int64_t stride = strides[trial % 3];
        std::vector<int64_t> sel((size_t)n);
        for (int i = 0; i < n; i++) sel[(size_t)i] = (int64_t)(rnd() % (uint32_t)n);
        std::vector<Row> rows((size_t)n);
        for (int k = 0; k < n; k++) {
            const int64_t *r = &idx[(size_t)sel[(size_t)k] * MIO_IDX_COLS];
            int64_t L = r[MIO_QUAL_LEN];
            if (max_len > 0 && L > max_len) L = max_len;
            rows[(size_t)k] = Row{r[MIO_SEQ_OFF], r[MIO_QUAL_OFF], (int32_t)L};
        }
        std::vector<uint8_t> first;
        for (int fill = 0; fill < 2; fill++) {
            std::vector<uint8_t> buf((size_t)cap + 64, fill ? (uint8_t)'N' : (uint8_t)0xff);
            uint8_t *base = buf.data() + (16 - ((uintptr_t)buf.data() & 15)) % 16;
            if (text_bytes) memcpy(base, text.data(), (size_t)text_bytes);
            g_lo = base; g_hi = base + cap;
            std::vector<uint8_t> out((size_t)n * stride, 0xAA), flags((size_t)n, 9);
            std::vector<int32_t> lens((size_t)n, -7);
            int64_t status[2] = {INT64_MAX, INT64_MAX};
            if (lower) pack_rows<true>(base, rows, offset, stride, out.data(), lens.data(), flags.data(), status);
            else pack_rows<false>(base, rows, offset, stride, out.data(), lens.data(), flags.data(), status);
            // the reference: mio_pack over the same selection; on a bad record it stops there, so the records before it are compared
            // from that call and every other record from a call of its own
            std::vector<uint8_t> ref((size_t)n * stride, 0xAA), rflags((size_t)n, 9);
            std::vector<int32_t> rlens((size_t)n, -7);
            int64_t bad = -1;
            const int32_t rc = mio_pack((const char *)base, idx.data(), sel.data(), n, offset, max_len, lower, stride, ref.data(),
                                        rlens.data(), rflags.data(), &bad);
            const int64_t mine = std::min(status[0], status[1]);
            if (rc == MIO_OK) {
                if (mine != INT64_MAX || out != ref || lens != rlens || flags != rflags) mismatches++;
            } else if (rc == MIO_E_RANGE) {
                const bool positive = strstr(mio_last_error(), "positive") != nullptr;
                if (mine != bad || positive != (status[0] == mine)) mismatches++;
                for (int k = 0; k < n; k++) {                     // every record that is clean by itself packs as the reference packs it
                    std::vector<uint8_t> one((size_t)stride); int32_t l1 = -1; uint8_t f1 = 9; int64_t b1 = -1;
                    if (mio_pack((const char *)base, idx.data(), &sel[(size_t)k], 1, offset, max_len, lower, stride, one.data(), &l1, &f1, &b1) != MIO_OK) continue;
                    if (memcmp(one.data(), &out[(size_t)k * stride], (size_t)stride) != 0 || l1 != lens[(size_t)k] || f1 != flags[(size_t)k]) mismatches++;
                }
            } else mismatches++;
            if (fill == 0) first = out; else if (first != out) mismatches++;
            cases++;
        }
    }
    printf("%ld cases, %ld loads out of bounds, %ld mismatches\n", cases, g_oob, mismatches);
    return (mismatches || g_oob) ? 1 : 0;
}
