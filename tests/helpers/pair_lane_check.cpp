// Host twin of the pairing kernels (moira_amd/csrc/mpb_pair_kernels.hip: k_pair_rows, k_pair_count, k_pair_scan, k_pair_lists):
// moira_amd/csrc/mpb_pair_lane.inc compiled for the host and run as the kernels run it -- workgroups of 256 lane states (four
// waves of 64) in lockstep, the ballots and the waves' counts computed from the lane states and handed to the lane code as
// arguments.  Every load is checked: an index element against the two index arrays (heap blocks of exactly their size), a text
// byte against the header range the lane code validated for that pair.  tests/test_pair_lane_model.py builds this program with
// the address and undefined-behaviour sanitizers, together with csrc/mpb_hostonly.cpp and csrc/fastio.cpp, and runs it.
//
// Per case it compares with mpb_pair_rows (one pair at a time, byte for byte on the row), with mio_first_header_mismatch, with
// the host's class and list construction (contigs_chunk's loops, restated here over the class table the test reads from
// mpb_contig.cpp) and with rec_cap = the largest need + 8.
//
// Input (argv[1]), little-endian: int32 cases; per case: char name[32]; int64 n_f, n_r, m, fbytes, rbytes; int32 maxabs, take,
// n_class, pad; int32 cap[16]; int64 fidx[n_f][6], ridx[n_r][6]; the two texts.
// Output: one line per case ("case NAME: ok mismatch=.. rowfail=.. built=.. rec_cap=.. longest=.. classes=..|.." or "case NAME: FAIL
// what"), then "<cases> cases, <x> loads out of bounds, <y> fail".  Exit status 3: a load out of bounds; 4: a comparison failed.
// Sensitivity builds (macros of this file alone, the lane code is untouched): -DPAIR_CHECK_WRONG_RANK hands the first lane of
// every wave but the first a rank one too high; -DPAIR_CHECK_SHORT_HDR compares the header tokens without their last byte.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "moira_io.h"
#include "moira_pb.h"

static const int64_t *g_fidx, *g_ridx;
static int64_t g_nf, g_nr;
static const uint8_t *g_ftext, *g_rtext;
static int64_t g_frange[2], g_rrange[2];                 // the header range of the pair at hand: offset, length
static long g_oob = 0;

static inline int64_t pr_ld_idx(const int64_t *idx, int64_t k)
{
    const int64_t rows = idx == g_fidx ? g_nf : idx == g_ridx ? g_nr : -1;
    if (k < 0 || k >= rows * 6) { g_oob++; return 0; }
    return idx[k];
}
static inline uint32_t pr_ldb(const uint8_t *text, int64_t i)
{
    const int64_t *range = text == g_ftext ? g_frange : text == g_rtext ? g_rrange : nullptr;
    if (!range || i < range[0] || i >= range[0] + range[1]) { g_oob++; return 0; }
    return text[i];
}

#define CD_FN static inline
static inline int cd_gload8(const uint8_t *p) { return *p; }
#include "mpb_contig_args.h"
#define PR_FN static inline
#define PR_LD_IDX(idx, k) pr_ld_idx(idx, k)
#define PR_LDB(text, i) pr_ldb(text, i)
#include "mpb_pair_lane.inc"

// the deliberately wrong comparison of the sensitivity build
static bool short_hdr_differs(const uint8_t *ftext, int64_t fho, int64_t fhl, const uint8_t *rtext, int64_t rho, int64_t rhl)
{
    if (fhl != rhl) return true;
    for (int64_t k = 0; k + 1 < fhl; k++)
        if (pr_ldb(ftext, fho + k) != pr_ldb(rtext, rho + k)) return true;
    return false;
}

template <typename T> static bool rd(FILE *f, T *p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: %s cases.bin\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int32_t n_cases = 0;
    if (!rd(f, &n_cases, 1)) return 2;
    long n_fail = 0;
    for (int cs = 0; cs < n_cases; cs++) {
        char name[33] = {0};
        int64_t h[5];
        int32_t t[4], cap[16];
        if (!rd(f, name, 32) || !rd(f, h, 5) || !rd(f, t, 4) || !rd(f, cap, 16)) { fprintf(stderr, "short case header\n"); return 2; }
        const int64_t n_f = h[0], n_r = h[1], m = h[2], fbytes = h[3], rbytes = h[4];
        const int maxabs = t[0], take = t[1], n_class = t[2];
        if (n_f < 0 || n_r < 0 || m < 0 || m > n_f || m > n_r || fbytes < 0 || rbytes < 0 || n_class < 1 || n_class > 16) { fprintf(stderr, "bad case header\n"); return 2; }
        // (new[] of the exact sizes: the sanitizer sees one element past either array)
        int64_t *fidx = new int64_t[(size_t)n_f * 6], *ridx = new int64_t[(size_t)n_r * 6];
        uint8_t *ftext = new uint8_t[(size_t)fbytes], *rtext = new uint8_t[(size_t)rbytes];
        if (!rd(f, fidx, (size_t)n_f * 6) || !rd(f, ridx, (size_t)n_r * 6) || !rd(f, ftext, (size_t)fbytes) || !rd(f, rtext, (size_t)rbytes)) { fprintf(stderr, "short case\n"); return 2; }
        g_fidx = fidx; g_ridx = ridx; g_nf = n_f; g_nr = n_r; g_ftext = ftext; g_rtext = rtext;
        MpbLdsClasses classes{};
        classes.n = n_class;
        for (int k = 0; k < n_class; k++) classes.cap[k] = cap[k];
        std::string why;
        auto bad = [&](const char *what, long long at) { if (why.empty()) why = std::string(what) + " at " + std::to_string(at); };

        // ---- k_pair_rows: one lane per pair
        std::vector<mpb_pair_row> rows((size_t)m);
        std::vector<int8_t> cls((size_t)m, -1);
        int64_t st_mis = INT64_MAX, st_row = INT64_MAX;
        for (int64_t i = 0; i < m; i++) {
            mpb_pair_row r;
            bool ok = pr_row(fidx, ridx, i, fbytes, rbytes, &r);
            int64_t rho, rhl;
            ok = pr_hdr_range(ridx, i, rbytes, &rho, &rhl) && ok;
            if (!ok) { r.l1 = 0; r.l2 = 0; }
            rows[(size_t)i] = r;
            cls[(size_t)i] = (int8_t)(ok ? pr_class(r, fbytes, rbytes, maxabs, take, classes) : -1);
            // the yardstick, one pair at a time (it stops at the first bad pair of a run)
            mpb_pair_row want;
            memset(&want, 0, sizeof(want));
            const int hrc = mpb_pair_rows(fidx + i * 6, ridx + i * 6, 1, fbytes, rbytes, INT64_MAX, &want, nullptr);
            const int64_t ro = ridx[i * 6 + 0], rl = ridx[i * 6 + 1];
            const bool rhdr_ok = ro >= 0 && rl >= 0 && rl <= rbytes && ro <= rbytes - rl;
            if (ok != (hrc == MPB_OK && rhdr_ok)) bad("mpb_pair_rows' verdict differs", i);
            if (ok && memcmp(&r, &want, sizeof(r)) != 0) bad("row differs from mpb_pair_rows'", i);
            if (!ok && cd_row_ok(r, fbytes, rbytes, INT64_MAX, maxabs)) bad("a refused pair's row passes cd_row_ok", i);
            if (!ok) { if (i < st_row) st_row = i; continue; }
            g_frange[0] = r.fhdr_off; g_frange[1] = r.hdr_len; g_rrange[0] = rho; g_rrange[1] = rhl;
#ifdef PAIR_CHECK_SHORT_HDR
            const bool differs = short_hdr_differs(ftext, r.fhdr_off, r.hdr_len, rtext, rho, rhl);
#else
            const bool differs = pr_hdr_differs(ftext, r.fhdr_off, r.hdr_len, rtext, rho, rhl);
            (void)short_hdr_differs;
#endif
            if (differs && i < st_mis) st_mis = i;
        }
        // mio_first_header_mismatch checks nothing: it runs over the pairs before the first refused one
        const int64_t n_ok = st_row == INT64_MAX ? m : st_row;
        const int64_t mis = st_mis < n_ok ? st_mis : -1;
        if (mis != mio_first_header_mismatch((const char *)ftext, fidx, (const char *)rtext, ridx, n_ok)) bad("mismatch differs from mio_first_header_mismatch's", mis);
        const int64_t nb = mis < 0 ? m : mis;
        char line[512];
        if (st_row < nb) {
            snprintf(line, sizeof(line), "refused mismatch=%lld rowfail=%lld built=0", (long long)mis, (long long)st_row);
        } else {
            // ---- k_pair_count, k_pair_scan, k_pair_lists over [0, nb)
            const int64_t groups = (nb + PR_LANES - 1) / PR_LANES;
            std::vector<uint32_t> table((size_t)groups * PR_CLASS_SLOTS, 0), prefix((size_t)groups * PR_CLASS_SLOTS, 0), wave_cnt((size_t)groups * 4 * PR_CLASS_SLOTS, 0);
            std::vector<unsigned long long> ballot((size_t)groups * 4 * PR_CLASS_SLOTS, 0);
            int64_t need_max = 0, longest = 0;
            for (int64_t i = 0; i < nb; i++) {
                const int64_t g = i / PR_LANES;
                const int wv = (int)(i % PR_LANES) / PR_WAVE, lane = (int)(i % PR_WAVE), c = cls[(size_t)i];
                if (pr_need(rows[(size_t)i]) > need_max) need_max = pr_need(rows[(size_t)i]);
                if (c < 0) continue;
                if ((int64_t)rows[(size_t)i].l1 + rows[(size_t)i].l2 > longest) longest = (int64_t)rows[(size_t)i].l1 + rows[(size_t)i].l2;
                ballot[(size_t)((g * 4 + wv) * PR_CLASS_SLOTS + c)] |= 1ull << lane;
                wave_cnt[(size_t)((g * 4 + wv) * PR_CLASS_SLOTS + c)]++;
                table[(size_t)(g * PR_CLASS_SLOTS + c)]++;
            }
            uint32_t head[2 * PR_CLASS_SLOTS] = {0};
            for (int k = 0; k < PR_CLASS_SLOTS; k++)
                for (int64_t g = 0; g < groups; g++) { prefix[(size_t)(g * PR_CLASS_SLOTS + k)] = head[k]; head[k] += table[(size_t)(g * PR_CLASS_SLOTS + k)]; }
            for (int k = 1; k < PR_CLASS_SLOTS; k++) head[PR_CLASS_SLOTS + k] = head[PR_CLASS_SLOTS + k - 1] + head[k - 1];
            std::vector<int32_t> list((size_t)nb, -1);
            for (int64_t i = 0; i < nb; i++) {
                const int64_t g = i / PR_LANES;
                const int wv = (int)(i % PR_LANES) / PR_WAVE, lane = (int)(i % PR_WAVE), c = cls[(size_t)i];
                if (c < 0) continue;
                uint32_t rank = pr_rank(ballot[(size_t)((g * 4 + wv) * PR_CLASS_SLOTS + c)], lane, &wave_cnt[(size_t)(g * 4 * PR_CLASS_SLOTS)], wv, c);
#ifdef PAIR_CHECK_WRONG_RANK
                if (wv > 0 && lane == 0) rank += 1;
#endif
                const int64_t at = pr_list_slot(head[PR_CLASS_SLOTS + c], prefix[(size_t)(g * PR_CLASS_SLOTS + c)], rank);
                if (at < 0 || at >= nb) { bad("list slot outside the list", i); continue; }
                if (list[(size_t)at] >= 0) bad("two pairs in one list slot", i);
                list[(size_t)at] = (int32_t)i;
            }
            // the host's construction (contigs_chunk, steps 3 and 4) with rec_cap = the largest need + 8
            const int64_t rec_cap = need_max + 8;
            const bool whole_back = !take || maxabs >= 30000;
            std::vector<int8_t> hcls((size_t)nb, -1);
            std::vector<int32_t> hlist((size_t)nb, -1);
            int64_t per_class[16] = {0}, first[16], fill[16], listed = 0, hlongest = 0, hneed = 0;
            for (int64_t i = 0; i < nb; i++) {
                const mpb_pair_row &r = rows[(size_t)i];
                hneed = r.hdr_len + 2 * ((int64_t)r.l1 + r.l2) > hneed ? r.hdr_len + 2 * ((int64_t)r.l1 + r.l2) : hneed;
            }
            for (int64_t i = 0; i < nb && !whole_back; i++) {
                if (!cd_row_ok(rows[(size_t)i], fbytes, rbytes, hneed + 8, maxabs)) continue;
                const int need = cd_lds_bytes(rows[(size_t)i].l1, rows[(size_t)i].l2);
                for (int k = 0; k < n_class; k++)
                    if (need <= cap[k]) { hcls[(size_t)i] = (int8_t)k; per_class[k]++; break; }
            }
            for (int k = 0; k < n_class; k++) { first[k] = fill[k] = listed; listed += per_class[k]; }
            for (int64_t i = 0; i < nb; i++)
                if (hcls[(size_t)i] >= 0) hlist[(size_t)fill[hcls[(size_t)i]]++] = (int32_t)i;
            for (int64_t k = 0; k < listed; k++) {
                const mpb_pair_row &r = rows[(size_t)hlist[(size_t)k]];
                if ((int64_t)r.l1 + r.l2 > hlongest) hlongest = (int64_t)r.l1 + r.l2;
            }
            if (rec_cap != hneed + 8) bad("rec_cap differs", rec_cap);
            if (longest != hlongest) bad("the longest l1 + l2 differs", longest);
            for (int64_t i = 0; i < nb; i++)
                if (cls[(size_t)i] != hcls[(size_t)i]) { bad("class differs from the host's", i); break; }
            for (int k = 0; k < n_class; k++)
                if ((int64_t)head[k] != per_class[k] || (int64_t)head[PR_CLASS_SLOTS + k] != first[k]) bad("class total or first place differs", k);
            for (int64_t k = 0; k < nb; k++)
                if (list[(size_t)k] != hlist[(size_t)k]) { bad("list entry differs from the host's", k); break; }
            std::string cl;
            for (int k = 0; k < n_class; k++) cl += (k ? "," : "") + std::to_string(per_class[k]);
            snprintf(line, sizeof(line), "ok mismatch=%lld rowfail=%lld built=%lld rec_cap=%lld longest=%lld classes=%s", (long long)mis,
                     (long long)(st_row == INT64_MAX ? -1 : st_row), (long long)nb, (long long)rec_cap, (long long)longest, cl.c_str());
        }
        if (!why.empty()) { n_fail++; printf("case %s: FAIL %s\n", name, why.c_str()); }
        else printf("case %s: %s\n", name, line);
        delete[] fidx; delete[] ridx; delete[] ftext; delete[] rtext;
    }
    fclose(f);
    printf("%d cases, %ld loads out of bounds, %ld fail\n", (int)n_cases, g_oob, n_fail);
    return g_oob ? 3 : n_fail ? 4 : 0;
}
