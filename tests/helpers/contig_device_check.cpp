// Host twin of k_contig (moira_amd/csrc/mpb_contig_kernels.hip): the per-lane code of moira_amd/csrc/mpb_contig_lane.inc compiled
// for the host and run as the wave runs it -- 64 lane states in lockstep, the neighbour's border cell handed over between steps,
// the two wave operations (maximum of the scan keys, prefix count of emitted columns) as loops over the lanes.  Every byte the
// lanes load from a text goes through a checked cd_gload8: a load outside [buf, buf + round_up(bytes, 16)) fails the run, and
// the bytes past the text are filled with 0xFF and with 'N' in turn (the results must not change).
// What this model shares with the kernel is the cd_* functions alone.  The order of the phases, the checks on K, the overlap
// window, the packing of the result words and the write-out in run_pair below are a second statement of contig_pair's, kept
// equal by hand: a change to the kernel's own glue is seen by tests/test_gpu_contigs.py on the device, not here.
//
// Input (argv[1]): a little-endian binary file written by tests/test_contig_device_model.py --
//   int32 n_cases; per case: int32 l1, l2, match, mismatch, gap, insert, deltaq, consensus, qcap, trim, offset, corrupt;
//                            l1 forward bases, l1 forward quality bytes, l2 reverse-read bases, l2 reverse-read quality bytes
//   (the reverse read as it lies in the FASTQ file: the kernel reverse-complements it).  corrupt != 0: the descriptor of the
//   case is damaged in way `corrupt` before the run; the pair must then be handed back without a single checked load failing.
// Output (argv[2]): per case  int32 done, aln_len, score, clen, overlap, gaps, mism;  aln_len bytes aln1, aln_len bytes aln2,
//   clen bytes contig, clen bytes q + offset.
// `check --lds out.bin` writes int32 MPB_CONTIG_LDS_MAX, CD_MAX_LEN and cd_lds_bytes(l1, l2) for l1, l2 = 1 .. CD_MAX_LEN (row l1),
//   so that a test can pick pairs on the size-class boundaries of mpb_contig.cpp without restating the layout.
// -DCD_CHECK_VARIANT=1 / 2 / 3 builds a deliberately WRONG model, to show that a fixture notices (tests/
//   test_contig_device_model.py): 1 the column wins the fix-up on cs >= rs, 2 the FIRST maximum of the last column / row instead
//   of the last, 3 the posterior tables clamped to qualities of 41 or less.  The lane code itself has no such switch.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "moira_pb.h"

static const uint8_t *g_lo[2], *g_hi[2];
static long g_oob = 0;
#define CD_FN static inline
static inline int cd_gload8(const uint8_t *p)
{
    if (!((p >= g_lo[0] && p < g_hi[0]) || (p >= g_lo[1] && p < g_hi[1]))) { g_oob++; return 0; }
    return *p;
}
#include "mpb_contig_args.h"

#ifndef CD_CHECK_VARIANT
#define CD_CHECK_VARIANT 0
#endif

#if CD_CHECK_VARIANT == 2
static uint32_t first_max_key(const int16_t *a, int n)
{
    int best = 0;
    for (int k = 1; k < n; k++) if (a[k] > a[best]) best = k;
    return ((uint32_t)((int)a[best] + 32768) << 16) | (uint32_t)best;
}
#endif

struct Result {
    int done = 0, aln_len = 0, score = 0, clen = 0, overlap = 0, gaps = 0, mism = 0;
    std::vector<uint8_t> aln1, aln2, contig, cq;
    bool operator==(const Result &o) const
    {
        return done == o.done && aln_len == o.aln_len && score == o.score && clen == o.clen && overlap == o.overlap && gaps == o.gaps &&
               mism == o.mism && aln1 == o.aln1 && aln2 == o.aln2 && contig == o.contig && cq == o.cq;
    }
};

// (lds: a heap block of exactly cd_lds_bytes(l1, l2) bytes, so that a host sanitizer build of this program sees any index past it)
template <int C>
static void run_pair(const mpb_pair_row &r, const uint8_t *ftext, const uint8_t *rtext, const CdParams &prm,
                     const int32_t *tabm, const int32_t *tabx, uint8_t *lds, int64_t rec_cap, Result &out)
{
    const CdShape sh = cd_shape(r.l1, r.l2);
    const CdLayout L = cd_layout(sh);
    int *hdr = (int *)(lds + L.hdr);
    uint32_t *col = (uint32_t *)(lds + L.col), *res = (uint32_t *)(lds + L.res);
    int16_t *lastcol = (int16_t *)(lds + L.lastcol), *lastrow = (int16_t *)(lds + L.lastrow);
    uint8_t *s1 = lds + L.s1, *s2 = lds + L.s2, *q1 = lds + L.q1, *q2 = lds + L.q2, *ptr = lds + L.ptr;
    bool ok = true;
    for (int lane = 0; lane < CD_LANES; lane++) ok &= cd_load_lane(r, ftext, rtext, prm.offset, lane, s1, s2, q1, q2);
    lastcol[0] = 0; lastrow[0] = 0;
    if (!ok) return;
    CdLane<C> st[CD_LANES];
    int outv[CD_LANES], shifted[CD_LANES];
    for (int lane = 0; lane < CD_LANES; lane++) { cd_lane_init<C>(st[lane], sh, s2, lane); outv[lane] = 0; }
    const int steps = cd_fill_steps(sh);
    for (int t = 0; t < steps; t++) {
        for (int lane = 0; lane < CD_LANES; lane++) shifted[lane] = lane ? outv[lane - 1] : 0;        // wave_shr:1, lane 0 reads 0
        for (int lane = 0; lane < CD_LANES; lane++)
            outv[lane] = cd_fill_step<C>(st[lane], sh, prm, lane, t, shifted[lane], outv[lane], s1, ptr, lastcol, lastrow);
    }
    uint32_t ck = 0, rk = 0;
    for (int lane = 0; lane < CD_LANES; lane++) {
        const uint32_t a = cd_scan_key(lastcol, sh.l1 + 1, lane), b = cd_scan_key(lastrow, sh.l2 + 1, lane);
        ck = a > ck ? a : ck; rk = b > rk ? b : rk;
    }
#if CD_CHECK_VARIANT == 2
    ck = first_max_key(lastcol, sh.l1 + 1); rk = first_max_key(lastrow, sh.l2 + 1);
#endif
    int bci, bri;
    int fix = cd_fixup(sh, ck, rk, &bci, &bri);
#if CD_CHECK_VARIANT == 1
    if (fix) fix = (ck >> 16) >= (rk >> 16) ? 1 : 2;
#endif
    cd_traceback<C>(sh, prm, s1, s2, ptr, lastcol, lastrow, fix, bci, bri, col, hdr);
    const int K = hdr[0], score = hdr[1], fstart = hdr[2], fend = hdr[3], rstart = hdr[4], rend = hdr[5];
    if (K < 1 || K > sh.l1 + sh.l2) return;
    int ostart, oend; bool reversed;
    if (fstart < rstart) { ostart = rstart; oend = fend; reversed = false; }
    else { ostart = fstart; oend = rend; reversed = true; }
    int clen = 0, gaps = 0, mism = 0;
    bool bad = false;
    for (int k0 = 0; k0 < K; k0 += CD_LANES) {
        uint32_t v[CD_LANES];
        for (int lane = 0; lane < CD_LANES; lane++) {
            const int k = k0 + lane;
            v[lane] = k < K ? cd_column(prm, s1, s2, q1, q2, tabm, tabx, col[K - 1 - k], k, ostart, oend, reversed) : 0;
        }
        int before = 0;
        for (int lane = 0; lane < CD_LANES; lane++) {
            const int k = k0 + lane;
            if (k < K) res[K - 1 - k] = v[lane] | ((uint32_t)(clen + before) << 20);
            before += (v[lane] & CD_EMIT) ? 1 : 0;
            gaps += (v[lane] & CD_GAP) ? 1 : 0; mism += (v[lane] & CD_MISM) ? 1 : 0; bad |= (v[lane] & CD_BAD) != 0;
        }
        clen += before;
    }
    if (bad) return;
    if ((int64_t)r.hdr_len + 2 * clen > rec_cap) { g_oob++; return; }
    out.contig.assign((size_t)clen, 0); out.cq.assign((size_t)clen, 0);
    out.aln1.assign((size_t)K, 0); out.aln2.assign((size_t)K, 0);
    for (int k = 0; k < K; k++) {
        const uint32_t v = res[K - 1 - k];
        if (v & CD_EMIT) {
            const int m = (int)(v >> 20);
            if (m < 0 || m >= clen) { g_oob++; continue; }
            out.contig[(size_t)m] = (uint8_t)(v >> 4); out.cq[(size_t)m] = (uint8_t)(v >> 12);
        }
        const uint32_t cv = col[K - 1 - k];
        const int i = (int)(cv & 0xffffu), j = (int)(cv >> 16);
        out.aln1[(size_t)k] = i ? s1[i - 1] : (uint8_t)'-';
        out.aln2[(size_t)k] = j ? s2[j - 1] : (uint8_t)'-';
    }
    out.done = 1; out.aln_len = K; out.score = score; out.clen = clen; out.overlap = oend - ostart; out.gaps = gaps; out.mism = mism;
}

static int32_t rd32(FILE *f) { int32_t v = 0; if (fread(&v, 4, 1, f) != 1) { fprintf(stderr, "short input\n"); exit(2); } return v; }

int main(int argc, char **argv)
{
    if (argc < 3) { fprintf(stderr, "usage: check cases.bin out.bin | check --lds out.bin\n"); return 2; }
    if (!strcmp(argv[1], "--lds")) {
        FILE *f = fopen(argv[2], "wb");
        if (!f) { fprintf(stderr, "cannot open files\n"); return 2; }
        const int32_t head[2] = {MPB_CONTIG_LDS_MAX, CD_MAX_LEN};
        fwrite(head, 4, 2, f);
        for (int l1 = 1; l1 <= CD_MAX_LEN; l1++)
            for (int l2 = 1; l2 <= CD_MAX_LEN; l2++) { const int32_t v = cd_lds_bytes(l1, l2); fwrite(&v, 4, 1, f); }
        fclose(f);
        return 0;
    }
    FILE *in = fopen(argv[1], "rb"), *outf = fopen(argv[2], "wb");
    if (!in || !outf) { fprintf(stderr, "cannot open files\n"); return 2; }
    std::vector<int32_t> tabs((size_t)2 * 65536);
    // the tables come from the library in the test (written in front of the cases)
    if (fread(tabs.data(), 4, tabs.size(), in) != tabs.size()) { fprintf(stderr, "short tables\n"); return 2; }
#if CD_CHECK_VARIANT == 3
    for (int t = 0; t < 2; t++)
        for (int a = 0; a < 256; a++)
            for (int b = 0; b < 256; b++) tabs[(size_t)t * 65536 + a * 256 + b] = tabs[(size_t)t * 65536 + std::min(a, 41) * 256 + std::min(b, 41)];
#endif
    const int n_cases = rd32(in);
    long handed = 0, differ = 0;
    for (int cs = 0; cs < n_cases; cs++) {
        int32_t h[12];
        for (int k = 0; k < 12; k++) h[k] = rd32(in);
        const int l1 = h[0], l2 = h[1], corrupt = h[11];
        CdParams prm;
        prm.match = h[2]; prm.mismatch = h[3]; prm.gap = h[4]; prm.insert = h[5]; prm.deltaq = h[6]; prm.consensus = h[7];
        prm.qcap = h[8]; prm.trim = h[9]; prm.offset = h[10];
        auto mag = [](int v) { return v < 0 ? -v : v; };
        prm.maxabs = std::max(mag(prm.match), std::max(mag(prm.mismatch), mag(prm.gap)));
        std::vector<uint8_t> fs((size_t)l1), fq((size_t)l1), rs((size_t)l2), rq((size_t)l2);
        if ((l1 && (fread(fs.data(), 1, (size_t)l1, in) != (size_t)l1 || fread(fq.data(), 1, (size_t)l1, in) != (size_t)l1)) ||
            (l2 && (fread(rs.data(), 1, (size_t)l2, in) != (size_t)l2 || fread(rq.data(), 1, (size_t)l2, in) != (size_t)l2))) { fprintf(stderr, "short case\n"); return 2; }
        // the two texts: "name\nseq\n+\nqual\n" at an odd offset, so that no line is aligned and the last ends the text
        auto make_text = [](const char *name, const std::vector<uint8_t> &s, const std::vector<uint8_t> &q, int64_t off[3]) {
            std::vector<uint8_t> t;
            t.push_back('@'); off[0] = (int64_t)t.size();
            for (const char *p = name; *p; p++) t.push_back((uint8_t)*p);
            t.push_back('\n'); off[1] = (int64_t)t.size(); t.insert(t.end(), s.begin(), s.end());
            t.push_back('\n'); t.push_back('+'); t.push_back('\n'); off[2] = (int64_t)t.size(); t.insert(t.end(), q.begin(), q.end());
            return t;
        };
        int64_t fo[3], ro[3];
        const std::vector<uint8_t> ft = make_text("pair_fwd", fs, fq, fo), rt = make_text("pr", rs, rq, ro);
        mpb_pair_row r{};
        r.fhdr_off = fo[0]; r.hdr_len = 8; r.fseq_off = fo[1]; r.fqual_off = fo[2]; r.rseq_off = ro[1]; r.rqual_off = ro[2]; r.l1 = l1; r.l2 = l2;
        const int64_t rec_cap = r.hdr_len + 2 * (int64_t)(l1 + l2) + 8;
        const int64_t fbytes = (int64_t)ft.size(), rbytes = (int64_t)rt.size();
        switch (corrupt) {
        case 0: break;
        case 1: r.fseq_off = fbytes - l1 + 1; break;
        case 2: r.fqual_off = -1; break;
        case 3: r.rseq_off = rbytes; break;
        case 4: r.rqual_off = (int64_t)1 << 40; break;
        case 5: r.l1 = CD_MAX_LEN + 1; break;
        case 6: r.l2 = 0; break;
        case 7: r.l2 = -5; break;
        case 8: r.hdr_len = (int32_t)rec_cap; break;
        case 9: r.fhdr_off = fbytes; break;
        case 10: r.l1 = 0x7fffffff; break;
        default: r.hdr_len = -1; break;
        }
        Result first;
        for (int fillv = 0; fillv < 2; fillv++) {
            const int64_t fcap = (fbytes + 15) / 16 * 16, rcap = (rbytes + 15) / 16 * 16;
            std::vector<uint8_t> fb((size_t)fcap, fillv ? (uint8_t)'N' : (uint8_t)0xff), rb((size_t)rcap, fillv ? (uint8_t)'N' : (uint8_t)0xff);
            memcpy(fb.data(), ft.data(), ft.size()); memcpy(rb.data(), rt.data(), rt.size());
            g_lo[0] = fb.data(); g_hi[0] = fb.data() + fcap; g_lo[1] = rb.data(); g_hi[1] = rb.data() + rcap;
            Result res;
            if (cd_row_ok(r, fbytes, rbytes, rec_cap, prm.maxabs)) {
                const int need = cd_lds_bytes(r.l1, r.l2);
                if (need <= MPB_CONTIG_LDS_MAX) {
                    std::vector<uint8_t> lds((size_t)need, 0xA5);
                    switch ((r.l2 + CD_LANES - 1) / CD_LANES) {
                    case 1: run_pair<1>(r, fb.data(), rb.data(), prm, tabs.data(), tabs.data() + 65536, lds.data(), rec_cap, res); break;
                    case 2: run_pair<2>(r, fb.data(), rb.data(), prm, tabs.data(), tabs.data() + 65536, lds.data(), rec_cap, res); break;
                    case 3: run_pair<3>(r, fb.data(), rb.data(), prm, tabs.data(), tabs.data() + 65536, lds.data(), rec_cap, res); break;
                    case 4: run_pair<4>(r, fb.data(), rb.data(), prm, tabs.data(), tabs.data() + 65536, lds.data(), rec_cap, res); break;
                    case 5: run_pair<5>(r, fb.data(), rb.data(), prm, tabs.data(), tabs.data() + 65536, lds.data(), rec_cap, res); break;
                    case 6: run_pair<6>(r, fb.data(), rb.data(), prm, tabs.data(), tabs.data() + 65536, lds.data(), rec_cap, res); break;
                    default: break;
                    }
                }
            }
            if (fillv == 0) first = res; else if (!(first == res)) differ++;
        }
        if (!first.done) handed++;
        const int32_t o[7] = {first.done, first.aln_len, first.score, first.clen, first.overlap, first.gaps, first.mism};
        fwrite(o, 4, 7, outf);
        if (first.aln_len) { fwrite(first.aln1.data(), 1, first.aln1.size(), outf); fwrite(first.aln2.data(), 1, first.aln2.size(), outf); }
        if (first.clen) { fwrite(first.contig.data(), 1, first.contig.size(), outf); fwrite(first.cq.data(), 1, first.cq.size(), outf); }
    }
    fclose(outf);
    printf("%d cases, %ld handed back, %ld loads out of bounds, %ld differ between fills\n", n_cases, handed, g_oob, differ);
    return (g_oob || differ) ? 1 : 0;
}
