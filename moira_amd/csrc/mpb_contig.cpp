// mpb_contig.cpp -- paired-read contigs on the device, behind the C ABI of libmoira_pb.so (include/moira_pb.h): the host entry that
// validates the pair descriptors (mpb_pair_rows, mpb_hostonly.cpp), uploads both texts once, buckets the pairs by the LDS their
// pointer matrix needs, launches k_contig (mpb_contig_kernels.hip) once per size class and brings the slots and arrays back.
// A pair the device does not take is handed back (done = 0); the caller builds it with libmoira_contig.so.
// mpb_contigs_filter_text_host is the same chunk call with the filter behind it: k_contig_rows hands the device's own index to
// k_pack_text, and mpb_filter_text_host's piece loop (filter_text_pieces, mpb_text.cpp) runs over the slots where they lie; the
// filter's results are queued (text_results_queue) with the contigs' own copies on the chunk's one StreamQueue (mpb_queue.h),
// behind one wait, and text_results_tail follows it.
// (Every mpb_* function defined here has C linkage: include/moira_pb.h declares it inside extern "C".)

#include "mpb_ctx.h"

#define CD_FN static inline
static inline int cd_gload8(const uint8_t *p) { return *p; }
#include "mpb_contig_args.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

namespace {

// LDS per wave of a launch: a 2 x 150 pair needs 11 KB, 2 x 250 21 KB, 2 x 300 42 KB, 2 x 384 57 KB (cd_lds_bytes).  A static
// worst case would leave two waves per CU.
const int32_t k_lds_class[] = {4096, 8192, 12288, 16384, 20480, 24576, 32768, 40960, 49152, MPB_CONTIG_LDS_MAX};
const int k_n_class = (int)(sizeof(k_lds_class) / sizeof(k_lds_class[0]));

struct ContigStage {
    uint8_t *ftext, *rtext; mpb_pair_row *rows; int32_t *list;
    uint8_t *out_buf; int64_t *out_idx; int32_t *overlap, *gaps, *mism; uint8_t *done;
    uint8_t *aln; int32_t *aln_len, *score;
    void layout(Carver &k, int64_t fbytes, int64_t rbytes, int64_t n, int64_t rec_cap, int64_t aln_cap)
    {
        k.take(ftext, align_up(fbytes > 0 ? fbytes : 1, 16));
        k.take(rtext, align_up(rbytes > 0 ? rbytes : 1, 16));
        k.take(rows, n); k.take(list, n);
        k.take(out_buf, align_up(n * rec_cap, 16)); k.take(out_idx, n * 6);     // (a text k_pack_text may read: whole 16-byte words)
        k.take(overlap, n); k.take(gaps, n); k.take(mism, n); k.take(done, n);
        k.take(aln, aln_cap > 0 ? 2 * n * aln_cap : 1); k.take(aln_len, aln_cap > 0 ? n : 1); k.take(score, aln_cap > 0 ? n : 1);
    }
};

int ensure_tables(mpb_ctx *c)
{
    if (c->contig_tabs_ready) return MPB_OK;
    std::vector<int32_t> t;
    try { t.resize((size_t)2 * 65536); } catch (const std::bad_alloc &) { return fail(MPB_E_NOMEM, "out of host memory for the posterior tables"); }
    int rc = mpb_contig_posterior_tables(t.data(), t.data() + 65536);
    if (rc) return rc;
    if ((rc = c->contig_tabs.grow(c, (int64_t)t.size() * 4))) return rc;
    if ((rc = copy_sync(c, c->contig_tabs.p, t.data(), t.size() * 4, hipMemcpyHostToDevice))) return rc;
    c->contig_tabs_ready = true;
    return MPB_OK;
}

// what mpb_contigs_filter_text_host asks for beyond the contigs: the filter of the slots where they lie
struct FilterAsk {
    int32_t max_len, lower_n_is_base; const mpb_filter_params *params; int32_t poisson;
    double *ee; int32_t *ns; uint8_t *pass; int32_t *len_out; uint8_t *flags_out; uint8_t *filtered;
    mpb_filter_counts *counts; int *filter_rc; int64_t *filter_bad_record;
};

// the chunk call of both entries (fa == nullptr: mpb_contigs_text_host)
int contigs_chunk(mpb_ctx *c, const char *ftext, int64_t ftext_bytes, const int64_t *fidx, const char *rtext,
                  int64_t rtext_bytes, const int64_t *ridx, int64_t n, int32_t fastq_offset,
                  const mpb_contig_params *params, int64_t rec_cap, char *out_buf, int64_t *out_idx, int32_t *overlap,
                  int32_t *gaps, int32_t *mismatches, uint8_t *done, char *aln_out, int64_t aln_cap,
                  int32_t *aln_len_out, int32_t *score_out, int64_t *n_done, int64_t *n_handed_back, int64_t *bad_record,
                  const FilterAsk *fa)
{
    CTXCHK(c);
    if (bad_record) *bad_record = -1;
    if (n_done) *n_done = 0;
    if (n_handed_back) *n_handed_back = 0;
    if (fa) {
        if (fa->filter_rc) *fa->filter_rc = MPB_OK;
        if (fa->filter_bad_record) *fa->filter_bad_record = -1;
        if (fa->counts) { fa->counts->n_reads = 0; fa->counts->n_pass = 0; fa->counts->n_fail = 0; fa->counts->n_overflow = 0; }
    }
    if (!params) return fail(MPB_E_INVALID, "params is NULL");
    if (n < 0 || ftext_bytes < 0 || rtext_bytes < 0 || rec_cap <= 0 || (ftext_bytes > 0 && !ftext) || (rtext_bytes > 0 && !rtext))
        return fail(MPB_E_INVALID, "mpb_contigs_text_host: bad arguments");
    if (n > 0x7fffffffll - 4096) return fail(MPB_E_INVALID, "chunk of %lld pairs exceeds 2^31; split it", (long long)n);
    if (n > 0 && (!fidx || !ridx || !out_buf || !out_idx || !overlap || !gaps || !mismatches || !done))
        return fail(MPB_E_INVALID, "NULL host buffer");
    if (fa && n > 0 && (!fa->ee || !fa->ns || !fa->pass || !fa->filtered)) return fail(MPB_E_INVALID, "NULL host buffer");
    if (fa && n > 0) memset(fa->filtered, 0, (size_t)n);
    if (aln_out && (aln_cap <= 0 || !aln_len_out || !score_out)) return fail(MPB_E_INVALID, "aln_out needs aln_cap > 0, aln_len_out and score_out");
    if (!aln_out) aln_cap = 0;
    // 1. the descriptors, validated on the host before anything is uploaded
    std::vector<mpb_pair_row> rows;
    std::vector<int32_t> list;
    std::vector<int8_t> cls;                             // the size class of a pair (-1: in no list)
    try { rows.resize((size_t)n); list.resize((size_t)n); cls.assign((size_t)n, -1); } catch (const std::bad_alloc &) { return fail(MPB_E_NOMEM, "out of host memory for %lld pair descriptors", (long long)n); }
    int rc = mpb_pair_rows(fidx, ridx, n, ftext_bytes, rtext_bytes, rec_cap, rows.data(), bad_record);
    if (rc) return rc;
    // 2. make_contig's parameter checks, with its messages
    if (params->insert <= 0) return fail(MPB_E_INVALID, "insert must be a positive integer");
    if (params->deltaq <= 0) return fail(MPB_E_INVALID, "deltaq must be a positive integer");
    if (params->qscore_cap < 0) return fail(MPB_E_INVALID, "qscore_cap must be a non-negative integer");
    if (params->consensus < 0 || params->consensus > 2) return fail(MPB_E_INVALID, "consensus_qscore must be \"best\", \"sum\" or \"posterior\".");
    if (fa && (rc = check_params(fa->params))) return rc;
    if (n == 0) return MPB_OK;
    auto mag = [](int32_t v) { return (int64_t)(v < 0 ? -(int64_t)v : v); };
    const int64_t maxabs = std::max(mag(params->match), std::max(mag(params->mismatch), mag(params->gap)));
    // 3. the size classes: the pairs the device takes, by the LDS their block needs (a pair outside 1..384 bases, or one whose scores
    // could leave 16 bits, is in no list: handed back)
    int64_t per_class[32] = {0};
    const bool whole_back = fastq_offset < 0 || fastq_offset > 255 || maxabs >= 30000;
    for (int64_t i = 0; i < n && !whole_back; i++) {
        if (!cd_row_ok(rows[(size_t)i], ftext_bytes, rtext_bytes, rec_cap, (int)maxabs)) continue;
        const int need = cd_lds_bytes(rows[(size_t)i].l1, rows[(size_t)i].l2);
        for (int k = 0; k < k_n_class; k++)
            if (need <= k_lds_class[k]) { cls[(size_t)i] = (int8_t)k; per_class[k]++; break; }
    }
    int64_t first[32], fill[32], listed = 0;
    for (int k = 0; k < k_n_class; k++) { first[k] = fill[k] = listed; listed += per_class[k]; }
    for (int64_t i = 0; i < n; i++)
        if (cls[(size_t)i] >= 0) list[(size_t)fill[cls[(size_t)i]]++] = (int32_t)i;
    if (listed == 0) {
        memset(done, 0, (size_t)n);
        if (n_handed_back) *n_handed_back = n;
        return MPB_OK;
    }
    if (params->consensus == 2 && (rc = ensure_tables(c))) return rc;
    // 4. the device block of the call (with a filter: the text call's block too, before anything is queued -- a block that
    // grows waits for the stream).  The row stride of the matrix is known here: no contig is longer than its pair's l1 + l2.
    ContigStage st{};
    if ((rc = carve(c, c->contig_stage, [&](Carver &k) { st.layout(k, ftext_bytes, rtext_bytes, n, rec_cap, aln_cap); }))) return rc;
    TextStage ts{};
    int64_t stride = 0, piece_rows = 0;
    if (fa) {
        int64_t longest = 0;
        for (int64_t k = 0; k < listed; k++) {
            const mpb_pair_row &r = rows[(size_t)list[(size_t)k]];
            longest = std::max(longest, (int64_t)r.l1 + r.l2);
        }
        if (fa->max_len > 0) longest = std::min(longest, (int64_t)fa->max_len);
        stride = align_up(std::max<int64_t>(longest, 1), 128);
        piece_rows = text_piece_rows(n, stride);
        if ((rc = carve(c, c->text_stage, [&](Carver &k) { ts.layout(k, 0, n, piece_rows, stride); }))) return rc;
    }
    hipStream_t s = c->stream;
    const int64_t fcap = align_up(ftext_bytes > 0 ? ftext_bytes : 1, 16), rcap = align_up(rtext_bytes > 0 ? rtext_bytes : 1, 16);
    // (the queue leaves before the vectors above and `fres`, which it copies from and into)
    TextResults fres{};
    if (fa) { fres.ee = fa->ee; fres.ns = fa->ns; fres.pass = fa->pass; fres.len = fa->len_out; fres.flags = fa->flags_out; }
    StreamQueue q(c);
    q.zero(st.ftext + ftext_bytes, fcap - ftext_bytes);
    q.zero(st.rtext + rtext_bytes, rcap - rtext_bytes);
    q.zero(st.done, n);
    q.up(st.ftext, ftext, ftext_bytes);
    q.up(st.rtext, rtext, rtext_bytes);
    q.up(st.rows, rows.data(), n * (int64_t)sizeof(mpb_pair_row));
    q.up(st.list, list.data(), listed * (int64_t)sizeof(int32_t));
    if (!q.ok()) return q.wait("hipMemcpyAsync (contig upload)");
    MpbContigArgs a{};
    a.ftext = st.ftext; a.fbytes = ftext_bytes; a.rtext = st.rtext; a.rbytes = rtext_bytes;
    a.rows = st.rows; a.n = n;
    a.prm.match = params->match; a.prm.mismatch = params->mismatch; a.prm.gap = params->gap; a.prm.insert = params->insert;
    a.prm.deltaq = params->deltaq; a.prm.consensus = params->consensus; a.prm.qcap = params->qscore_cap;
    a.prm.trim = params->trim_overlap ? 1 : 0; a.prm.offset = fastq_offset; a.prm.maxabs = (int)maxabs;
    a.rec_cap = rec_cap;
    a.tab_match = params->consensus == 2 ? (const int32_t *)c->contig_tabs.p : nullptr;
    a.tab_mism = a.tab_match ? a.tab_match + 65536 : nullptr;
    a.out_buf = st.out_buf; a.out_idx = st.out_idx; a.overlap = st.overlap; a.gaps = st.gaps; a.mism = st.mism; a.done = st.done;
    a.aln_out = aln_out ? st.aln : nullptr; a.aln_cap = aln_cap; a.aln_len = st.aln_len; a.score = st.score;
    // 5. one launch per size class
    for (int k = 0; k < k_n_class; k++) {
        if (!per_class[k]) continue;
        a.list = st.list + first[k]; a.count = per_class[k]; a.lds_cap = k_lds_class[k];
        q.run(MPB_K_CONTIG, [&] { mpb_launch_contigs(a, s); });
    }
    // 5b. the filter of the slots where they lie: the device's own index becomes k_pack_text's descriptors (k_contig_rows, behind
    // the launches above on the same stream), then mpb_filter_text_host's piece loop over the slot buffer.  A quality out of
    // range or a filter call that fails leaves the contigs valid: it is reported beside them, and nothing counts as filtered.
    int frc = MPB_OK;
    int64_t f_pass = 0, f_overflow = 0, f_bad = -1;
    char f_msg[MPB_ERR_LEN] = "";
    const bool host_tail = fa && text_host_tail(fa->params, fa->poisson);
    if (fa) q.run(MPB_K_CONTIG_ROWS, [&] { mpb_launch_contig_rows(st.out_idx, st.done, n, rec_cap, fa->max_len, stride, ts.rows, s); });
    if (fa && q.ok()) {
        frc = filter_text_pieces(q, st.out_buf, n * rec_cap, ts.rows, n, stride, piece_rows, fastq_offset, fa->lower_n_is_base,
                                 fa->params, fa->poisson, ts, &f_pass, &f_overflow, &f_bad);
        if (frc != MPB_OK && frc != MPB_E_RANGE && frc != MPB_E_INVALID) return frc;
        if (frc) { strncpy(f_msg, mpb_last_error(), sizeof(f_msg) - 1); }
    }
    // 6. the slots and arrays
    if (fa && frc == MPB_OK && (rc = text_results_queue(q, ts, n, host_tail, fres))) return rc;
    q.down(out_buf, st.out_buf, n * rec_cap);
    q.down(out_idx, st.out_idx, n * 6 * (int64_t)sizeof(int64_t));
    q.down(overlap, st.overlap, n * (int64_t)sizeof(int32_t));
    q.down(gaps, st.gaps, n * (int64_t)sizeof(int32_t));
    q.down(mismatches, st.mism, n * (int64_t)sizeof(int32_t));
    q.down(done, st.done, n);
    if (aln_out) {
        q.down(aln_out, st.aln, 2 * n * aln_cap);
        q.down(aln_len_out, st.aln_len, n * (int64_t)sizeof(int32_t));
        q.down(score_out, st.score, n * (int64_t)sizeof(int32_t));
    }
    if ((rc = q.wait("k_contig / hipMemcpyAsync (contig results)"))) return rc;
    int64_t nd = 0;
    for (int64_t i = 0; i < n; i++) nd += done[i] != 0;
    if (n_done) *n_done = nd;
    if (n_handed_back) *n_handed_back = n - nd;
    if (!fa) return MPB_OK;
    // 7. the filter's outcome per pair: a pair counts as filtered when the device built it and the chunk's filter went through
    if (frc != MPB_OK) {
        if (fa->filter_rc) *fa->filter_rc = frc;
        if (f_bad >= 0) {                                // a position in pair order -> in the order of the built pairs, as a
            int64_t rank = 0;                            // mpb_filter_text_host call over them would have counted it
            for (int64_t i = 0; i < f_bad && i < n; i++) rank += done[i] != 0;
            f_bad = rank;
        }
        if (fa->filter_bad_record) *fa->filter_bad_record = f_bad;
        (void)fail(frc, "%s", f_msg);                    // mpb_last_error() holds the filter's message
        return MPB_OK;
    }
    if ((rc = text_results_tail(n, fa->params, host_tail, fres, nullptr))) return rc;
    int64_t np = 0;
    for (int64_t i = 0; i < n; i++) {
        fa->filtered[i] = done[i] != 0;
        np += done[i] != 0 && fa->pass[i] != 0;
    }
    (void)f_pass;                                        // (the pieces' own count includes the empty rows of handed-back pairs)
    if (fa->counts) { fa->counts->n_reads = nd; fa->counts->n_pass = np; fa->counts->n_fail = nd - np; fa->counts->n_overflow = f_overflow; }
    return MPB_OK;
}

}  // namespace

int mpb_contigs_text_host(mpb_ctx *c, const char *ftext, int64_t ftext_bytes, const int64_t *fidx, const char *rtext,
                          int64_t rtext_bytes, const int64_t *ridx, int64_t n, int32_t fastq_offset,
                          const mpb_contig_params *params, int64_t rec_cap, char *out_buf, int64_t *out_idx, int32_t *overlap,
                          int32_t *gaps, int32_t *mismatches, uint8_t *done, char *aln_out, int64_t aln_cap,
                          int32_t *aln_len_out, int32_t *score_out, int64_t *n_done, int64_t *n_handed_back, int64_t *bad_record)
{
    return contigs_chunk(c, ftext, ftext_bytes, fidx, rtext, rtext_bytes, ridx, n, fastq_offset, params, rec_cap, out_buf, out_idx,
                         overlap, gaps, mismatches, done, aln_out, aln_cap, aln_len_out, score_out, n_done, n_handed_back, bad_record,
                         nullptr);
}

int mpb_contigs_filter_text_host(mpb_ctx *c, const char *ftext, int64_t ftext_bytes, const int64_t *fidx, const char *rtext,
                                 int64_t rtext_bytes, const int64_t *ridx, int64_t n, int32_t fastq_offset,
                                 const mpb_contig_params *params, int64_t rec_cap, char *out_buf, int64_t *out_idx, int32_t *overlap,
                                 int32_t *gaps, int32_t *mismatches, uint8_t *done, char *aln_out, int64_t aln_cap,
                                 int32_t *aln_len_out, int32_t *score_out, int64_t *n_done, int64_t *n_handed_back, int64_t *bad_record,
                                 int32_t max_len, int32_t lower_n_is_base, const mpb_filter_params *filter_params, int32_t poisson,
                                 double *ee, int32_t *ns, uint8_t *pass, int32_t *len_out, uint8_t *flags_out, uint8_t *filtered,
                                 mpb_filter_counts *counts, int *filter_rc, int64_t *filter_bad_record)
{
    const FilterAsk fa{max_len, lower_n_is_base, filter_params, poisson, ee, ns, pass, len_out, flags_out, filtered, counts,
                       filter_rc, filter_bad_record};
    return contigs_chunk(c, ftext, ftext_bytes, fidx, rtext, rtext_bytes, ridx, n, fastq_offset, params, rec_cap, out_buf, out_idx,
                         overlap, gaps, mismatches, done, aln_out, aln_cap, aln_len_out, score_out, n_done, n_handed_back, bad_record,
                         &fa);
}
