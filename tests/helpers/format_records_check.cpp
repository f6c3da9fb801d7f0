// format_records_check.cpp -- the lane code of mpb_format_records_host (moira_amd/csrc/mpb_format_lane.inc with FM_LD_U64: the report
// kind, the ee suffix, aux) on the host, built with -fsanitize=address,undefined together with csrc/fastio.cpp and run as a
// program (tests/test_format_records_model.py).  As format_lane_check.cpp: 256 lane states in lockstep, FM_GROUP lanes per
// record; every load is checked against its array (ee: nsel words, by position; aux: three arrays of stride 3 inside
// int32[n_records][3], by record), every store against the record's own range [prefix[k], prefix[k + 1]) and against a second
// store to the same byte.  The result is compared byte for byte with mio_format(ee) or, for kind 4, mio_format_report.
//   format_records_check cases.bin   ->  "case NAME: ok bytes=N" | "case NAME: refused rowfail=K" | "case NAME: FAIL what"
// Exit 4 when a case fails.  -DFM_WRONG_TIES_HALF_UP / -DFM_WRONG_AUX_SIGN: the sensitivity builds.

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "moira_io.h"

static const uint8_t *g_text, *g_blob;
static int64_t g_text_cap;
static const int64_t *g_idx, *g_sel, *g_ri;
static const int32_t *g_lab, *g_aux;
static const uint64_t *g_ee;
static int64_t g_idx_n, g_nsel, g_aux_n;
static int64_t g_bad_loads, g_bad_stores, g_twice;

struct fm_w16;
static fm_w16 ld16(const uint8_t *base, int64_t off);
static int64_t ld_i64(const int64_t *p, int64_t k)
{
    const int64_t n = p == g_idx ? g_idx_n : (p == g_sel || p == g_ri) ? g_nsel : -1;
    if (k < 0 || k >= n) { g_bad_loads++; return 0; }
    return p[k];
}
static int32_t ld_i32(const int32_t *p, int64_t k)
{
    if (p && p == g_lab) {
        if (k < 0 || k >= g_nsel) { g_bad_loads++; return 0; }
        return p[k];
    }
    if (g_aux && p >= g_aux && p < g_aux + 3) {                // one of the three arrays inside aux[n_records][3]
        if (k < 0 || k > g_aux_n - 3 || k % 3 != 0) { g_bad_loads++; return 0; }
        return p[k];
    }
    g_bad_loads++;
    return 0;
}
static uint64_t ld_u64(const uint64_t *p, int64_t k)
{
    if (!p || p != g_ee || k < 0 || k >= g_nsel) { g_bad_loads++; return 0; }
    return p[k];
}

struct CheckedOut { uint8_t *p; uint8_t *seen; int64_t lo, hi; };
static void st8(CheckedOut &o, int64_t pos, uint32_t b)
{
    if (pos < o.lo || pos >= o.hi) { g_bad_stores++; return; }
    if (o.seen[pos]) g_twice++;
    o.seen[pos] = 1;
    o.p[pos] = (uint8_t)b;
}

#define FM_FN static inline
#define FM_LD_I64(p, k) ld_i64((p), (k))
#define FM_LD_I32(p, k) ld_i32((p), (k))
#define FM_LD_U64(p, k) ld_u64((p), (k))
#define FM_LD16(text, off) ld16((text), (off))
#define FM_ST8(o, pos, b) st8((o), (pos), (b))
#include "mpb_format_lane.inc"

static fm_w16 ld16(const uint8_t *base, int64_t off)
{
    fm_w16 o;
    memset(&o, 0, sizeof(o));
    const int64_t cap = base == g_text ? g_text_cap : base == g_blob ? FM_BLOB_BYTES : -1;
    if ((off & 15) || off < 0 || off + 16 > cap) { g_bad_loads++; return o; }
    memcpy(o.w, base + off, 16);
    return o;
}

struct Reader {
    std::vector<uint8_t> d; size_t at = 0;
    template <typename T> T get() { T v; memcpy(&v, d.data() + at, sizeof(T)); at += sizeof(T); return v; }
    const uint8_t *bytes(size_t n) { const uint8_t *p = d.data() + at; at += n; return p; }
};

struct CaseHead {
    char name[32];
    int64_t n_records, text_bytes, nsel;
    int32_t has_sel, kind, fastq_offset, out_offset, clamp_q0, max_len, has_relabel, relabel_len, n_labels, has_label_id, has_ee, has_aux;
};

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
        // (exactly as many elements as the arrays hold: a load past them is also the sanitizer's; an empty index still has an address)
        std::vector<int64_t> idx(h.n_records ? (size_t)h.n_records * 6 : 1), sel((size_t)h.nsel), ri((size_t)h.nsel);
        std::vector<int32_t> lab((size_t)h.nsel), aux(h.n_records ? (size_t)h.n_records * 3 : 1);
        std::vector<uint64_t> ee((size_t)h.nsel);
        std::vector<double> eed((size_t)h.nsel);
        if (h.n_records) memcpy(idx.data(), in.bytes((size_t)h.n_records * 48), (size_t)h.n_records * 48);
        const int64_t cap = (h.text_bytes + 15) / 16 * 16;
        uint8_t *text = (uint8_t *)malloc((size_t)(cap > 0 ? cap : 1));      // exactly the words the kernel may ask for
        memset(text, 0, (size_t)(cap > 0 ? cap : 1));
        memcpy(text, in.bytes((size_t)h.text_bytes), (size_t)h.text_bytes);
        if (h.has_sel && h.nsel) memcpy(sel.data(), in.bytes((size_t)h.nsel * 8), (size_t)h.nsel * 8);
        std::string relabel((const char *)in.bytes((size_t)h.relabel_len), (size_t)h.relabel_len);
        if (h.has_relabel && h.nsel) memcpy(ri.data(), in.bytes((size_t)h.nsel * 8), (size_t)h.nsel * 8);
        std::vector<std::string> labels;
        for (int i = 0; i < h.n_labels; i++) { const int32_t n = in.get<int32_t>(); labels.emplace_back((const char *)in.bytes((size_t)n), (size_t)n); }
        if (h.has_label_id && h.nsel) memcpy(lab.data(), in.bytes((size_t)h.nsel * 4), (size_t)h.nsel * 4);
        if (h.has_ee && h.nsel) { memcpy(ee.data(), in.bytes((size_t)h.nsel * 8), (size_t)h.nsel * 8); memcpy(eed.data(), ee.data(), (size_t)h.nsel * 8); }
        if (h.has_aux && h.n_records) memcpy(aux.data(), in.bytes((size_t)h.n_records * 12), (size_t)h.n_records * 12);
        std::vector<uint8_t> blob(FM_BLOB_BYTES, 0);
        FmParams p;
        memset(&p, 0, sizeof(p));
        p.n_records = h.n_records; p.text_bytes = h.text_bytes; p.kind = h.kind; p.fastq_offset = h.fastq_offset;
        p.out_offset = h.out_offset; p.floor_q = h.clamp_q0 ? 1 : 0; p.max_len = h.max_len;
        p.has_relabel = h.has_relabel; p.has_labels = h.has_label_id; p.n_labels = h.has_label_id ? h.n_labels : 0;
        p.has_ee = h.has_ee; p.aux_stride = 3;
        if (h.has_relabel) { memcpy(blob.data(), relabel.data(), relabel.size()); p.str_len[0] = (uint8_t)relabel.size(); }
        for (int i = 0; i < h.n_labels; i++) {
            memcpy(blob.data() + (size_t)(1 + i) * FM_SLOT, labels[(size_t)i].data(), labels[(size_t)i].size());
            p.str_len[1 + i] = (uint8_t)labels[(size_t)i].size();
        }
        g_text = text; g_text_cap = cap; g_blob = blob.data(); g_idx = idx.data(); g_idx_n = h.n_records * 6;
        g_sel = h.has_sel ? sel.data() : nullptr; g_ri = h.has_relabel ? ri.data() : nullptr; g_lab = h.has_label_id ? lab.data() : nullptr;
        g_ee = h.has_ee ? ee.data() : nullptr; g_aux = h.has_aux ? aux.data() : nullptr; g_aux_n = h.n_records * 3;
        g_nsel = h.nsel; g_bad_loads = 0; g_bad_stores = 0; g_twice = 0;
        const int32_t *a0 = g_aux, *a1 = g_aux ? g_aux + 1 : nullptr, *a2 = g_aux ? g_aux + 2 : nullptr;
        const int per = FM_LANES / FM_GROUP;
        // k_fmt_count: the workgroups one after the other, the lanes of one in lockstep
        std::vector<int64_t> size((size_t)h.nsel + 1, 0), prefix((size_t)h.nsel + 2, 0);
        int64_t status = INT64_MAX;
        for (int64_t g0 = 0; g0 < h.nsel; g0 += per) {
            FmRow row[FM_LANES]; FmExtra ex[FM_LANES]; bool ok[FM_LANES]; uint64_t cnt[FM_LANES];
            for (int t = 0; t < FM_LANES; t++) {
                const int64_t k = g0 + t / FM_GROUP;
                ok[t] = false; cnt[t] = 0;
                if (k >= h.nsel) continue;
                ok[t] = fm_rec_row(idx.data(), g_sel, g_ri, g_lab, g_ee, a0, a1, a2, k, p, &row[t], &ex[t]);
                if (ok[t] && p.kind == FM_KIND_QUAL) cnt[t] = fm_count_lane(text, row[t], t % FM_GROUP, p);
            }
            for (int t = 0; t < FM_LANES; t += FM_GROUP) {
                const int64_t k = g0 + t / FM_GROUP;
                if (k >= h.nsel) continue;
                uint64_t sum = 0;
                for (int j = 0; j < FM_GROUP; j++) sum += cnt[t + j];
                size[(size_t)k] = ok[t] ? fm_size_x(row[t], ex[t], sum, p) : 0;
                if (!ok[t] && k < status) status = k;
            }
        }
        for (int64_t k = 0; k < h.nsel; k++) prefix[(size_t)k + 1] = prefix[(size_t)k] + size[(size_t)k];
        const int64_t total = prefix[(size_t)h.nsel];
        std::string what;
        if (status != INT64_MAX) {
            if (g_bad_loads) { what = "loads out of bounds while refusing"; }
            else { printf("case %s: refused rowfail=%lld\n", h.name, (long long)status); free(text); continue; }
        }
        std::vector<uint8_t> out((size_t)total + 1, 0), seen((size_t)total + 1, 0);
        if (what.empty()) {
            // k_fmt_write
            for (int64_t g0 = 0; g0 < h.nsel; g0 += per) {
                FmRow row[FM_LANES]; FmExtra ex[FM_LANES]; int64_t w[FM_LANES];
                const int lanes = (int)std::min<int64_t>(FM_LANES, (h.nsel - g0) * FM_GROUP);
                for (int t = 0; t < lanes; t++) {
                    const int64_t k = g0 + t / FM_GROUP;
                    fm_rec_row(idx.data(), g_sel, g_ri, g_lab, g_ee, a0, a1, a2, k, p, &row[t], &ex[t]);
                    CheckedOut o{out.data(), seen.data(), prefix[(size_t)k], prefix[(size_t)k + 1]};
                    w[t] = prefix[(size_t)k] + fm_write_header_x(text, blob.data(), row[t], ex[t], t % FM_GROUP, p, o, prefix[(size_t)k]);
                    if (p.kind == FM_KIND_REPORT) continue;
                    if (p.kind != FM_KIND_QUAL) fm_write_lines(text, row[t], t % FM_GROUP, p, o, w[t]);
                }
                if (p.kind != FM_KIND_QUAL) continue;
                for (int t0 = 0; t0 < lanes; t0 += FM_GROUP) {
                    const int64_t k = g0 + t0 / FM_GROUP;
                    CheckedOut o{out.data(), seen.data(), prefix[(size_t)k], prefix[(size_t)k + 1]};
                    const FmRow &r = row[t0];
                    int64_t base = w[t0];
                    const int steps = (r.L + 16 * FM_GROUP - 1) / (16 * FM_GROUP);
                    for (int s = 0; s < steps; s++) {
                        fm_w16 ql[FM_GROUP]; int nv[FM_GROUP], mine[FM_GROUP];
                        for (int j = 0; j < FM_GROUP; j++) {
                            ql[j] = fm_qual_word(text, r, s, j, &nv[j]);
                            mine[j] = fm_qual_bytes16(ql[j], nv[j], s == 0 && j == 0, p);
                        }
                        int before = 0;
                        for (int j = 0; j < FM_GROUP; j++) {
                            fm_qual_render16(ql[j], nv[j], s == 0 && j == 0, p, o, base + before);
                            before += mine[j];
                        }
                        base += before;
                    }
                    st8(o, base, '\n');
                }
            }
            if (g_bad_loads) what = "loads out of bounds";
            else if (g_bad_stores) what = "stores outside the record's range";
            else if (g_twice) what = "a byte stored twice";
            else if ((int64_t)std::count(seen.begin(), seen.begin() + total, 1) != total) what = "a byte of the output was never stored";
        }
        if (what.empty()) {
            std::vector<const char *> labp;
            for (auto &s : labels) labp.push_back(s.c_str());
            std::vector<char> ref((size_t)total * 4 + 256 + (size_t)h.nsel * 64);
            int64_t needed = -1, got;
            if (h.kind == FM_KIND_REPORT)
                got = mio_format_report((const char *)text, idx.data(), g_sel, h.nsel, h.has_relabel ? relabel.c_str() : nullptr, g_ri,
                                        h.has_ee ? eed.data() : nullptr, aux.data(), ref.data(), (int64_t)ref.size(), &needed);
            else
                got = mio_format((const char *)text, idx.data(), g_sel, h.nsel, h.kind, h.fastq_offset, h.out_offset, h.clamp_q0,
                                 h.max_len, h.has_relabel ? relabel.c_str() : nullptr, g_ri, h.has_ee ? eed.data() : nullptr,
                                 h.has_label_id ? labp.data() : nullptr, g_lab, ref.data(), (int64_t)ref.size(), &needed);
            if (got != total) what = "the host formatter writes " + std::to_string((long long)got) + " bytes, the lanes count " + std::to_string((long long)total);
            else if (memcmp(ref.data(), out.data(), (size_t)total) != 0) {
                int64_t at = 0;
                while (ref[(size_t)at] == (char)out[(size_t)at]) at++;
                char hex[8];
                what = "byte " + std::to_string((long long)at) + " differs from the host formatter's:";
                for (int64_t i = at; i < total && i < at + 8; i++) { snprintf(hex, sizeof(hex), " %02x", (unsigned)out[(size_t)i]); what += hex; }
                what += " for";
                for (int64_t i = at; i < total && i < at + 8; i++) { snprintf(hex, sizeof(hex), " %02x", (unsigned)(uint8_t)ref[(size_t)i]); what += hex; }
            }
        }
        all_bad_loads += g_bad_loads;
        if (what.empty()) printf("case %s: ok bytes=%lld\n", h.name, (long long)total);
        else { printf("case %s: FAIL %s\n", h.name, what.c_str()); fails++; }
        free(text);
    }
    printf("%d cases, %lld loads out of bounds, %d fail\n", n_cases, (long long)all_bad_loads, fails);
    return fails ? 4 : 0;
}
