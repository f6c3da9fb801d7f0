// collapse_lane_check.cpp -- the collapse kernels' lane code (moira_amd/csrc/mpb_collapse_lane.inc) on the host, built with
// -fsanitize=address,undefined together with csrc/fastio.cpp and run as a program (tests/test_collapse_lane_model.py).  One lane
// per record, CL_LANES lane states in lockstep: k_col_hash over a workgroup, then k_col_group with every lane of a workgroup
// taking ONE step of its probe walk (one modelled atomic) per round until all have settled, then k_col_rep.  Every load is
// checked against its array (the text: whole 16-byte words below round_up(text_bytes, 16), which is also all the buffer holds),
// every store against its array; the compare-and-swap and the minimum are modelled on plain words.  Each case runs twice: the
// records handed to the lanes in order, and in a seeded shuffled order (which changes who owns a slot).  hash must be
// mio_py2_hash's, rep the first record with the same truncated bytes (made here by a map), and both equal between the two runs.
// forge 1: before the group step every hash[] entry becomes one value; forge 2: values that differ between sequences but start
// every probe walk at one slot -- the group step reads hash[] as an input, so this pins its byte compare and its walk.
// Behind every case whose hashes are not forged, mio_collapse_add_grouped takes the lanes' arrays (verify on) under the same
// sanitizers, in two chunks, beside mio_collapse_add: the same groups.
//   collapse_lane_check cases.bin   ->  "case NAME: ok n=N groups=G" | "case NAME: refused rowfail=K" | "case NAME: FAIL what"
// Exit 4 when a case fails.  -DCL_SKIP_BYTE_COMPARE / -DCL_NO_MAX_LEN_CLAMP: the sensitivity builds.

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <string>
#include <vector>

#include "moira_io.h"

static const uint8_t *g_text;
static int64_t g_text_cap, g_n, g_cap;
static const int64_t *g_idx;
static const uint64_t *g_hash;
static const int32_t *g_table, *g_rep;
static const uint32_t *g_first;
static const int64_t *g_slot;
static int64_t g_bad_loads, g_bad_stores;

template <typename T> static T ld(const T *p, int64_t k, const void *want, int64_t n)
{
    if ((const void *)p != want || k < 0 || k >= n) { g_bad_loads++; return T(0); }
    return p[k];
}
template <typename T, typename V> static void st(T *p, int64_t k, V v, const void *want, int64_t n)
{
    if ((const void *)p != want || k < 0 || k >= n) { g_bad_stores++; return; }
    p[k] = (T)v;
}
static int32_t cas32(int32_t *p, int64_t s, int32_t want, int32_t v)
{
    if (p != g_table || s < 0 || s >= g_cap) { g_bad_stores++; return 0; }
    const int32_t seen = p[s];
    if (seen == want) p[s] = v;
    return seen;
}
static void min32(uint32_t *p, int64_t s, uint32_t v)
{
    if (p != g_first || s < 0 || s >= g_cap) { g_bad_stores++; return; }
    if (v < p[s]) p[s] = v;
}

struct cl_w16;
static cl_w16 ld16(const uint8_t *base, int64_t off);

#define CL_FN static inline
#define CL_LD_I64(p, k) ld((p), (k), g_idx, g_n * 6)
#define CL_LD_U64(p, k) ld((p), (k), g_hash, g_n)
#define CL_LD_U32(p, k) ld((p), (k), g_first, g_cap)
#define CL_LD_SLOT(p, k) ld((p), (k), g_slot, g_n)
#define CL_LD16(text, off) ld16((text), (off))
#define CL_ST_U64(p, k, v) st((p), (k), (v), g_hash, g_n)
#define CL_ST_I32(p, k, v) st((p), (k), (v), g_rep, g_n)
#define CL_ST_SLOT(p, k, v) st((p), (k), (v), g_slot, g_n)
#define CL_CAS_I32(p, s, want, v) cas32((p), (s), (want), (v))
#define CL_MIN_U32(p, s, v) min32((p), (s), (v))
#include "mpb_collapse_lane.inc"

static cl_w16 ld16(const uint8_t *base, int64_t off)
{
    cl_w16 o;
    memset(&o, 0, sizeof(o));
    if (base != g_text || (off & 15) || off < 0 || off + 16 > g_text_cap) { g_bad_loads++; return o; }
    memcpy(o.w, base + off, 16);
    return o;
}

struct Reader {
    std::vector<uint8_t> d; size_t at = 0;
    template <typename T> T get() { T v; memcpy(&v, d.data() + at, sizeof(T)); at += sizeof(T); return v; }
    const uint8_t *bytes(size_t n) { const uint8_t *p = d.data() + at; at += n; return p; }
};

struct CaseHead { char name[32]; int64_t n_records, text_bytes; int32_t max_len, forge; };

struct Result { std::vector<uint64_t> hash; std::vector<int32_t> rep; int64_t status; };

static uint64_t inverse(uint64_t a)               // of an odd a modulo 2^64 (Newton: the right bits double with every step)
{
    uint64_t x = a;
    for (int i = 0; i < 6; i++) x *= 2 - a * x;
    return x;
}

// the three kernels over the records in the order `order` hands them to the lanes
static Result run_lanes(const uint8_t *text, const int64_t *idx, ClParams p, int forge, const std::vector<int64_t> &order)
{
    const int64_t n = p.n_records;
    Result r;
    r.hash.assign((size_t)n + 1, 0); r.rep.assign((size_t)n + 1, -7); r.status = INT64_MAX;
    std::vector<int32_t> table((size_t)p.cap, CL_EMPTY);
    std::vector<uint32_t> first((size_t)p.cap, 0xffffffffu);
    std::vector<int64_t> slot((size_t)n + 1, -7);
    g_hash = r.hash.data(); g_rep = r.rep.data(); g_table = table.data(); g_first = first.data(); g_slot = slot.data(); g_cap = p.cap;
    for (int64_t g0 = 0; g0 < n; g0 += CL_LANES)             // k_col_hash
        for (int64_t t = g0; t < std::min<int64_t>(g0 + CL_LANES, n); t++) {
            const int64_t k = order[(size_t)t];
            ClRow row;
            const bool ok = cl_row(idx, k, p, &row);
            CL_ST_U64(r.hash.data(), k, ok ? cl_hash(text, row) : 0ull);
            if (!ok && k < r.status) r.status = k;
        }
    if (r.status != INT64_MAX) return r;
    std::vector<uint64_t> real(r.hash);
    if (forge == 1) std::fill(r.hash.begin(), r.hash.begin() + n, 0x123456789abcdefull);
    if (forge == 2) {                                        // start slot 5 for everybody, the low bits of the real hash keep them apart
        const uint64_t inv = inverse(0x9E3779B97F4A7C15ull), low = ((uint64_t)1 << p.cap_shift) - 1;
        for (int64_t k = 0; k < n; k++) r.hash[(size_t)k] = inv * (((uint64_t)5 << p.cap_shift) | (real[(size_t)k] & low));
    }
    for (int64_t g0 = 0; g0 < n; g0 += CL_LANES) {           // k_col_group: the lanes of a workgroup one step each, round by round
        const int lanes = (int)std::min<int64_t>(CL_LANES, n - g0);
        ClProbe w[CL_LANES]; bool walking[CL_LANES];
        for (int t = 0; t < lanes; t++) { cl_probe_begin(idx, r.hash.data(), order[(size_t)(g0 + t)], p, &w[t]); walking[t] = true; }
        for (bool any = true; any;) {
            any = false;
            for (int t = 0; t < lanes; t++)
                if (walking[t]) { walking[t] = cl_probe_step(text, idx, r.hash.data(), order[(size_t)(g0 + t)], p, table.data(), &w[t]); any = any || walking[t]; }
        }
        for (int t = 0; t < lanes; t++) cl_probe_end(order[(size_t)(g0 + t)], w[t], first.data(), slot.data());
    }
    for (int64_t t = 0; t < n; t++) cl_rep(first.data(), slot.data(), order[(size_t)t], r.rep.data());      // k_col_rep
    if (forge) r.hash = real;
    return r;
}

// mio_collapse_add and mio_collapse_add_grouped on two objects, chunk by chunk: the same groups in the same order
static std::string grouped_entry(const uint8_t *text, const int64_t *idx, int64_t n, int32_t max_len, const Result &r)
{
    mio_collapse *a = mio_collapse_create(), *b = mio_collapse_create();
    std::string what;
    std::vector<double> ee((size_t)n + 1);
    for (int64_t k = 0; k < n; k++) ee[(size_t)k] = (double)((k * 7919) % 13) / 4;
    const int64_t cut = n / 3;
    for (int part = 0; part < 2 && what.empty(); part++) {
        const int64_t lo = part ? cut : 0, m = part ? n - cut : cut;
        std::vector<int32_t> rep((size_t)m + 1);
        for (int64_t k = 0; k < m; k++) rep[(size_t)k] = r.rep[(size_t)(lo + k)] >= lo ? (int32_t)(r.rep[(size_t)(lo + k)] - lo) : (int32_t)k;
        if (mio_collapse_add(a, (const char *)text, idx + lo * 6, m, max_len, ee.data() + lo, nullptr, nullptr)) what = "mio_collapse_add fails";
        else if (mio_collapse_add_grouped(b, (const char *)text, idx + lo * 6, m, max_len, ee.data() + lo, nullptr, nullptr, r.hash.data() + lo,
                                          rep.data(), 1))
            what = std::string("mio_collapse_add_grouped refuses the lanes' arrays: ") + mio_last_error();
    }
    if (what.empty()) {
        const int64_t g = mio_collapse_count(a);
        std::vector<double> ea((size_t)g + 1), eb((size_t)g + 1);
        std::vector<int64_t> la((size_t)g + 1), lb((size_t)g + 1), sa((size_t)g + 1), sb((size_t)g + 1);
        if (mio_collapse_count(b) != g) what = "the grouped entry makes another number of groups";
        else if (mio_collapse_export(a, ea.data(), la.data(), sa.data(), nullptr, nullptr) || mio_collapse_export(b, eb.data(), lb.data(), sb.data(), nullptr, nullptr))
            what = "mio_collapse_export fails";
        else if (ea != eb || la != lb || sa != sb) what = "the grouped entry's groups differ from mio_collapse_add's";
    }
    mio_collapse_destroy(a);
    mio_collapse_destroy(b);
    return what;
}

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    Reader in;
    {
        FILE *f = fopen(argv[1], "rb");
        if (!f) return 2;
        fseek(f, 0, SEEK_END);
        const long n = ftell(f);
        fseek(f, 0, SEEK_SET);
        in.d.resize((size_t)n);
        if (fread(in.d.data(), 1, (size_t)n, f) != (size_t)n) return 2;
        fclose(f);
    }
    const int n_cases = in.get<int32_t>();
    int fails = 0;
    int64_t all_bad_loads = 0;
    for (int ci = 0; ci < n_cases; ci++) {
        const CaseHead h = in.get<CaseHead>();
        const int64_t n = h.n_records;
        std::vector<int64_t> idx((size_t)n * 6 + 1);
        memcpy(idx.data(), in.bytes((size_t)n * 48), (size_t)n * 48);
        const int64_t cap = (h.text_bytes + 15) / 16 * 16;
        uint8_t *text = (uint8_t *)malloc((size_t)(cap > 0 ? cap : 1));      // exactly the words the kernels may ask for
        memset(text, 0, (size_t)(cap > 0 ? cap : 1));
        memcpy(text, in.bytes((size_t)h.text_bytes), (size_t)h.text_bytes);
        ClParams p;
        memset(&p, 0, sizeof(p));
        p.n_records = n; p.text_bytes = h.text_bytes; p.max_len = h.max_len;
        p.cap_shift = 60;                                    // (mpb_collapse_text_host's sizing)
        while (((int64_t)1 << (64 - p.cap_shift)) < 2 * n) p.cap_shift--;
        p.cap = (int64_t)1 << (64 - p.cap_shift);
        g_text = text; g_text_cap = cap; g_idx = idx.data(); g_n = n; g_bad_loads = 0; g_bad_stores = 0;
        std::vector<int64_t> order((size_t)n);
        for (int64_t k = 0; k < n; k++) order[(size_t)k] = k;
        const Result r1 = run_lanes(text, idx.data(), p, h.forge, order);
        std::mt19937_64 rng(12345 + (uint64_t)ci);
        std::shuffle(order.begin(), order.end(), rng);
        const Result r2 = run_lanes(text, idx.data(), p, h.forge, order);
        std::string what;
        if (g_bad_loads) what = "loads out of bounds";
        else if (g_bad_stores) what = "stores or atomics outside their array";
        else if (r1.status != r2.status) what = "the two orders refuse different records";
        else if (r1.status != INT64_MAX) { printf("case %s: refused rowfail=%lld\n", h.name, (long long)r1.status); free(text); continue; }
        int64_t groups = 0;
        if (what.empty()) {
            std::vector<uint64_t> ref((size_t)n + 1);
            if (mio_py2_hash((const char *)text, idx.data(), n, h.max_len, ref.data())) what = "mio_py2_hash fails";
            std::map<std::string, int32_t> seen;
            for (int64_t k = 0; k < n && what.empty(); k++) {
                int64_t L = idx[(size_t)k * 6 + 3];
                if (h.max_len > 0 && L > h.max_len) L = h.max_len;
                const int32_t want = seen.emplace(std::string((const char *)text + idx[(size_t)k * 6 + 2], (size_t)L), (int32_t)k).first->second;
                if (r1.hash[(size_t)k] != ref[(size_t)k]) what = "hash[" + std::to_string((long long)k) + "] is not mio_py2_hash's";
                else if (r1.rep[(size_t)k] != want)
                    what = "rep[" + std::to_string((long long)k) + "] = " + std::to_string(r1.rep[(size_t)k]) + ", the first equal record is " + std::to_string(want);
                else if (r2.hash[(size_t)k] != r1.hash[(size_t)k] || r2.rep[(size_t)k] != r1.rep[(size_t)k])
                    what = "record " + std::to_string((long long)k) + " differs between the two orders";
            }
            groups = (int64_t)seen.size();
        }
        if (what.empty() && !h.forge) what = grouped_entry(text, idx.data(), n, h.max_len, r1);
        all_bad_loads += g_bad_loads;
        if (what.empty()) printf("case %s: ok n=%lld groups=%lld\n", h.name, (long long)n, (long long)groups);
        else { printf("case %s: FAIL %s\n", h.name, what.c_str()); fails++; }
        free(text);
    }
    printf("%d cases, %lld loads out of bounds, %d fail\n", n_cases, (long long)all_bad_loads, fails);
    return fails ? 4 : 0;
}
