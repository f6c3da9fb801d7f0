// mpb_contig.cpp -- paired-read contigs on the device, behind the C ABI of libmoira_pb.so (include/moira_pb.h): the host entry that
// validates the pair descriptors (mpb_pair_rows, mpb_hostonly.cpp), uploads both texts once, buckets the pairs by the LDS their
// pointer matrix needs, launches k_contig (mpb_contig_kernels.hip) once per size class and brings the slots and arrays back.
// A pair the device does not take is handed back (done = 0); the caller builds it with libmoira_contig.so.
// mpb_contigs_filter_text_host is the same chunk call with the filter behind it: k_contig_rows hands the device's own index to
// k_pack_text, and mpb_filter_text_host's piece loop (filter_text_pieces, mpb_text.cpp) runs over the slots where they lie; the
// filter's results are queued (text_results_queue) with the contigs' own copies on the chunk's one StreamQueue (mpb_queue.h),
// behind one wait, and text_results_tail follows it.
// mpb_contigs_filter_fastq_host is that call from the two texts ALONE: both record indexes are built on the device
// (mpb_index_kernels.hip), the pairing step (mpb_pair_kernels.hip) turns them into the descriptors and class lists where they lie,
// and the chunk call runs from there.  contigs_chunk is therefore two halves: "descriptors and lists from the host indexes"
// (contigs_chunk itself, which uploads them) and "run from descriptors and lists that lie on the device" (contigs_run).
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
    // n_in: the pairs whose descriptors and list entries the block holds (0, with no text: they lie elsewhere on the device)
    void layout(Carver &k, int64_t fbytes, int64_t rbytes, int64_t n_in, int64_t n, int64_t rec_cap, int64_t aln_cap)
    {
        k.take(ftext, align_up(fbytes > 0 ? fbytes : 1, 16));
        k.take(rtext, align_up(rbytes > 0 ? rbytes : 1, 16));
        k.take(rows, n_in); k.take(list, n_in);
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

// make_contig's parameter checks, with its messages, then the filter's
int check_contig_params(const mpb_contig_params *params, const FilterAsk *fa)
{
    if (params->insert <= 0) return fail(MPB_E_INVALID, "insert must be a positive integer");
    if (params->deltaq <= 0) return fail(MPB_E_INVALID, "deltaq must be a positive integer");
    if (params->qscore_cap < 0) return fail(MPB_E_INVALID, "qscore_cap must be a non-negative integer");
    if (params->consensus < 0 || params->consensus > 2) return fail(MPB_E_INVALID, "consensus_qscore must be \"best\", \"sum\" or \"posterior\".");
    return fa ? check_params(fa->params) : MPB_OK;
}

int64_t contig_maxabs(const mpb_contig_params *params)
{
    auto mag = [](int32_t v) { return (int64_t)(v < 0 ? -(int64_t)v : v); };
    return std::max(mag(params->match), std::max(mag(params->mismatch), mag(params->gap)));
}

// a chunk of which the device takes no pair at all: a fastq_offset or scores outside what k_contig computes with
bool contig_whole_back(int32_t fastq_offset, int64_t maxabs) { return fastq_offset < 0 || fastq_offset > 255 || maxabs >= 30000; }

// The descriptors and class lists of a chunk as they lie on the device, whoever wrote them: the host (contigs_chunk uploads them
// into the contig stage beside the texts) or the pairing kernels (mpb_contigs_filter_fastq_host: the texts lie in the index's stage)
struct ContigWork {
    const uint8_t *ftext, *rtext; int64_t fbytes, rbytes;
    const mpb_pair_row *rows; const int32_t *list;
    int64_t per_class[32], first[32];
    int64_t longest;                                     // the largest l1 + l2 of a listed pair: no contig is longer
};

// The device blocks of the call (with a filter: the text call's block too, before anything is queued -- a block that grows waits
// for the stream).  The row stride of the matrix is known here: no contig is longer than its pair's l1 + l2.
int contig_blocks(mpb_ctx *c, ContigStage &st, TextStage &ts, int64_t fbytes, int64_t rbytes, int64_t n_in, int64_t n, int64_t rec_cap,
                  int64_t aln_cap, int64_t longest, const FilterAsk *fa, int64_t *stride, int64_t *piece_rows)
{
    int rc;
    if ((rc = carve(c, c->contig_stage, [&](Carver &k) { st.layout(k, fbytes, rbytes, n_in, n, rec_cap, aln_cap); }))) return rc;
    *stride = 0; *piece_rows = 0;
    if (fa) {
        if (fa->max_len > 0) longest = std::min(longest, (int64_t)fa->max_len);
        *stride = align_up(std::max<int64_t>(longest, 1), 128);
        *piece_rows = text_piece_rows(n, *stride);
        if ((rc = carve(c, c->text_stage, [&](Carver &k) { ts.layout(k, 0, n, *piece_rows, *stride); }))) return rc;
    }
    return MPB_OK;
}

// The second half of the chunk call: run from descriptors and lists that lie on the device (w), into the blocks contig_blocks
// laid out.  One k_contig launch per non-empty class, the filter of the slots where they lie, the copies back (`also` queues what
// else the caller wants behind the same wait), the last wait and the counts.
template <typename Also>
int contigs_run(StreamQueue &q, const ContigWork &w, const ContigStage &st, const TextStage &ts, int64_t stride, int64_t piece_rows,
                int64_t n, int32_t fastq_offset, const mpb_contig_params *params, int64_t maxabs, int64_t rec_cap, char *out_buf,
                int64_t *out_idx, int32_t *overlap, int32_t *gaps, int32_t *mismatches, uint8_t *done, char *aln_out, int64_t aln_cap,
                int32_t *aln_len_out, int32_t *score_out, int64_t *n_done, int64_t *n_handed_back, const FilterAsk *fa, TextResults &fres,
                Also &&also)
{
    mpb_ctx *c = q.c;
    hipStream_t s = c->stream;
    int rc;
    MpbContigArgs a{};
    a.ftext = w.ftext; a.fbytes = w.fbytes; a.rtext = w.rtext; a.rbytes = w.rbytes;
    a.rows = w.rows; a.n = n;
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
        if (!w.per_class[k]) continue;
        a.list = w.list + w.first[k]; a.count = w.per_class[k]; a.lds_cap = k_lds_class[k];
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
    also(q);
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

void filter_ask_reset(const FilterAsk *fa)
{
    if (!fa) return;
    if (fa->filter_rc) *fa->filter_rc = MPB_OK;
    if (fa->filter_bad_record) *fa->filter_bad_record = -1;
    if (fa->counts) { fa->counts->n_reads = 0; fa->counts->n_pass = 0; fa->counts->n_fail = 0; fa->counts->n_overflow = 0; }
}

// The chunk call of the two entries that bring their record indexes (fa == nullptr: mpb_contigs_text_host).  The first half:
// descriptors and lists from the host indexes, uploaded beside the texts; contigs_run is the second.
int contigs_chunk(mpb_ctx *c, const char *ftext, int64_t ftext_bytes, const int64_t *fidx, const char *rtext,
                  int64_t rtext_bytes, const int64_t *ridx, int64_t n, int32_t fastq_offset,
                  const mpb_contig_params *params, int64_t rec_cap, char *out_buf, int64_t *out_idx, int32_t *overlap,
                  int32_t *gaps, int32_t *mismatches, uint8_t *done, char *aln_out, int64_t aln_cap,
                  int32_t *aln_len_out, int32_t *score_out, int64_t *n_done, int64_t *n_handed_back, int64_t *bad_record,
                  const FilterAsk *fa)
{
    CTXCHK(c);
    resident_drop_contigs(c);                                // (the slot block may grow or be overwritten; a single-end text stays)
    if (bad_record) *bad_record = -1;
    if (n_done) *n_done = 0;
    if (n_handed_back) *n_handed_back = 0;
    filter_ask_reset(fa);
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
    if ((rc = check_contig_params(params, fa))) return rc;
    if (n == 0) return MPB_OK;
    const int64_t maxabs = contig_maxabs(params);
    // 3. the size classes: the pairs the device takes, by the LDS their block needs (a pair outside 1..384 bases, or one whose scores
    // could leave 16 bits, is in no list: handed back)
    ContigWork w{};
    const bool whole_back = contig_whole_back(fastq_offset, maxabs);
    for (int64_t i = 0; i < n && !whole_back; i++) {
        if (!cd_row_ok(rows[(size_t)i], ftext_bytes, rtext_bytes, rec_cap, (int)maxabs)) continue;
        const int need = cd_lds_bytes(rows[(size_t)i].l1, rows[(size_t)i].l2);
        for (int k = 0; k < k_n_class; k++)
            if (need <= k_lds_class[k]) { cls[(size_t)i] = (int8_t)k; w.per_class[k]++; break; }
    }
    int64_t fill[32], listed = 0;
    for (int k = 0; k < k_n_class; k++) { w.first[k] = fill[k] = listed; listed += w.per_class[k]; }
    for (int64_t i = 0; i < n; i++)
        if (cls[(size_t)i] >= 0) list[(size_t)fill[cls[(size_t)i]]++] = (int32_t)i;
    if (listed == 0) {
        memset(done, 0, (size_t)n);
        if (n_handed_back) *n_handed_back = n;
        return MPB_OK;
    }
    if (params->consensus == 2 && (rc = ensure_tables(c))) return rc;
    // 4. the device blocks of the call
    for (int64_t k = 0; fa && k < listed; k++) {
        const mpb_pair_row &r = rows[(size_t)list[(size_t)k]];
        w.longest = std::max(w.longest, (int64_t)r.l1 + r.l2);
    }
    ContigStage st{};
    TextStage ts{};
    int64_t stride = 0, piece_rows = 0;
    if ((rc = contig_blocks(c, st, ts, ftext_bytes, rtext_bytes, n, n, rec_cap, aln_cap, w.longest, fa, &stride, &piece_rows))) return rc;
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
    w.ftext = st.ftext; w.fbytes = ftext_bytes; w.rtext = st.rtext; w.rbytes = rtext_bytes; w.rows = st.rows; w.list = st.list;
    return contigs_run(q, w, st, ts, stride, piece_rows, n, fastq_offset, params, maxabs, rec_cap, out_buf, out_idx, overlap, gaps,
                       mismatches, done, aln_out, aln_cap, aln_len_out, score_out, n_done, n_handed_back, fa, fres, [](StreamQueue &) {});
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

namespace {

// what the pairing kernels write, beside the two record indexes in the context's index block: descriptors, classes and list of the
// m candidate pairs, the count table and its prefix per workgroup of 256 pairs, the head words and the status
struct PairStage {
    mpb_pair_row *rows; int8_t *cls; int32_t *list; uint32_t *table, *prefix, *head; int64_t *status;
    void layout(Carver &k, int64_t m)
    {
        const int64_t groups = (m + 255) / 256;
        k.take(rows, m > 0 ? m : 1); k.take(cls, m > 0 ? m : 1); k.take(list, m > 0 ? m : 1);
        k.take(table, (groups > 0 ? groups : 1) * 16); k.take(prefix, (groups > 0 ? groups : 1) * 16);
        k.take(head, MPB_PAIR_HEAD_WORDS); k.take(status, 4);
    }
};

// one text's share of the read-back behind k_fq_rows: the records before the first bad one, the rows written
bool index_verdict(const int64_t *status, int64_t cand, Indexed &in)
{
    if (status[2] != 0) return false;
    if (status[0] != INT64_MAX && (status[0] < 0 || status[0] >= cand)) return false;
    in.n = status[0] == INT64_MAX ? cand : status[0];
    in.rows = status[0] == INT64_MAX ? cand : in.n + 1;
    return true;
}

}  // namespace

int mpb_contigs_filter_fastq_host(mpb_ctx *c, const char *ftext, int64_t ftext_bytes, int32_t ffinal, const char *rtext,
                                  int64_t rtext_bytes, int32_t rfinal, int64_t max_records, int32_t fastq_offset,
                                  const mpb_contig_params *params, int64_t *fidx_out, int64_t *ridx_out, int64_t idx_cap_rows,
                                  int64_t *n_f, int32_t *f_bad_kind, int64_t *n_r, int32_t *r_bad_kind, int64_t *n_pairs,
                                  int64_t *mismatch, int64_t *n_built, int64_t *f_consumed, int64_t *r_consumed, int32_t *why,
                                  int32_t *which, int64_t *rec_cap_out, char *out_buf, int64_t out_cap_bytes, int64_t *out_idx,
                                  int32_t *overlap, int32_t *gaps, int32_t *mismatches, uint8_t *done, int64_t *n_done,
                                  int64_t *n_handed_back, int32_t max_len, int32_t lower_n_is_base,
                                  const mpb_filter_params *filter_params, int32_t poisson, double *ee, int32_t *ns, uint8_t *pass,
                                  int32_t *len_out, uint8_t *flags_out, uint8_t *filtered, mpb_filter_counts *counts, int *filter_rc,
                                  int64_t *filter_bad_record)
{
    // 1. the arguments first: what is wrong with them is said with or without a device
    int filter_rc_here = MPB_OK;                             // (whether the filter went through decides what stays resident)
    int64_t back_here = 0;
    if (!filter_rc) filter_rc = &filter_rc_here;
    if (!n_handed_back) n_handed_back = &back_here;
    const FilterAsk fa{max_len, lower_n_is_base, filter_params, poisson, ee, ns, pass, len_out, flags_out, filtered, counts,
                       filter_rc, filter_bad_record};
    if (n_done) *n_done = 0;
    if (n_handed_back) *n_handed_back = 0;
    filter_ask_reset(&fa);
    if (!params) return fail(MPB_E_INVALID, "params is NULL");
    if (ftext_bytes < 0 || rtext_bytes < 0 || (ftext_bytes > 0 && !ftext) || (rtext_bytes > 0 && !rtext) || max_records < 0 || max_len < 0 ||
        idx_cap_rows < 1 || out_cap_bytes < 0 || !fidx_out || !ridx_out || !n_f || !f_bad_kind || !n_r || !r_bad_kind || !n_pairs ||
        !mismatch || !n_built || !f_consumed || !r_consumed || !why || !which || !rec_cap_out)
        return fail(MPB_E_INVALID, "mpb_contigs_filter_fastq_host: bad arguments");
    if (!out_buf || !out_idx || !overlap || !gaps || !mismatches || !done || !ee || !ns || !pass || !filtered)
        return fail(MPB_E_INVALID, "NULL host buffer");
    int rc;
    if ((rc = check_text_bytes(ftext_bytes)) || (rc = check_text_bytes(rtext_bytes))) return rc;
    if ((rc = check_contig_params(params, &fa))) return rc;
    CTXCHK(c);
    resident_drop(c);                                        // (both texts' shares are carved out of the index's two blocks)
    *n_f = 0; *n_r = 0; *f_bad_kind = 0; *r_bad_kind = 0; *n_pairs = 0; *mismatch = -1; *n_built = 0; *f_consumed = 0; *r_consumed = 0;
    *why = MPB_FQ_WHY_TAKEN; *which = 0; *rec_cap_out = 8;
    const int64_t maxabs = contig_maxabs(params);
    const bool whole_back = contig_whole_back(fastq_offset, maxabs);
    hipStream_t s = c->stream;
    const int64_t bytes[2] = {ftext_bytes, rtext_bytes};
    const char *const text[2] = {ftext, rtext};
    const int32_t final_text[2] = {ffinal, rfinal};
    int64_t tiles[2], cand[2];
    for (int t = 0; t < 2; t++) tiles[t] = (bytes[t] + MPB_FQ_TILE - 1) / MPB_FQ_TILE;
    uint32_t *const pin_head[2] = {c->pin->fq_head, c->pin->fq_head2};
    int64_t *const pin_status[2] = {c->pin->fq_status, c->pin->fq_status2};
    int64_t *pst = c->pin->pair_status;
    Indexed in[2];
    PairStage ps{};
    // (the queue leaves before `fres`, which it copies into)
    TextResults fres{ee, ns, pass, len_out, flags_out, {}};
    StreamQueue q(c);
    // 2. both texts, each uploaded once into one block neither can move the other in; lines and their scan; one wait for both heads
    if ((rc = carve(c, c->fastq_stage, [&](Carver &k) { for (int t = 0; t < 2; t++) in[t].st.layout(k, bytes[t], tiles[t]); }))) return rc;
    for (int t = 0; t < 2; t++) {
        q.zero(in[t].st.text + bytes[t], align_up(bytes[t] > 0 ? bytes[t] : 1, 16) - bytes[t]);      // (k_contig reads whole words)
        q.up(in[t].st.text, text[t], bytes[t]);
        fastq_index_queue_head(q, in[t], bytes[t], final_text[t], pin_head[t]);
    }
    if ((rc = q.wait("hipMemcpyAsync (text upload) / k_fq_lines / k_fq_scan"))) return rc;
    for (int t = 0; t < 2; t++) {
        if (pin_head[t][1] & 2u) { *why = MPB_FQ_WHY_LONE_CR; *which = t; return MPB_OK; }
        if (pin_head[t][1] & 1u) { *why = MPB_FQ_WHY_NON_ASCII; *which = t; return MPB_OK; }
    }
    for (int t = 0; t < 2; t++) {
        const int64_t lines = pin_head[t][2];
        cand[t] = lines / 4 < max_records ? lines / 4 : max_records;
    }
    *n_f = cand[0]; *n_r = cand[1];
    for (int t = 0; t < 2; t++)
        if (cand[t] + 1 > idx_cap_rows)
            return fail(MPB_E_INVALID, "idx_cap_rows %lld is too small: the %s text holds %lld records, and the row after them may be written",
                        (long long)idx_cap_rows, t ? "reverse" : "forward", (long long)cand[t]);
    *n_f = 0; *n_r = 0;
    const int64_t m = std::min(cand[0], cand[1]);            // the candidate pairs
    for (int t = 0; t < 2; t++) {
        Carver size;
        in[t].ix.layout(size, 4 * cand[t] + 1, cand[t] > 0 ? cand[t] : 1);
        if (size.bytes() > MPB_FQ_INDEX_MAX_BYTES) { *why = MPB_FQ_WHY_LINE_TABLE; *which = t; return MPB_OK; }
    }
    rc = carve(c, c->fastq_index, [&](Carver &k) {
        for (int t = 0; t < 2; t++) in[t].ix.layout(k, 4 * cand[t] + 1, cand[t] > 0 ? cand[t] : 1);
        ps.layout(k, m);
    });
    if (rc == MPB_E_NOMEM) { *why = MPB_FQ_WHY_LINE_TABLE; return MPB_OK; }
    if (rc) return rc;
    // 3. line starts and rows of each text, the pairing behind them; one wait for the three status blocks.  (k_fq_rows' second
    // pass over the records before a bad one only finds their longest packed length, which nothing here asks for.)
    for (int t = 0; t < 2; t++) {
        if (cand[t] == 0) { pin_status[t][0] = INT64_MAX; pin_status[t][1] = pin_status[t][2] = pin_status[t][3] = 0; continue; }
        FastqStage &st = in[t].st;
        FastqIndex &ix = in[t].ix;
        const int64_t n_start = 4 * cand[t] + 1, count = cand[t], tb = bytes[t], nt = tiles[t];
        q.run(MPB_K_FQ_STARTS, [&] { mpb_launch_fq_starts(st.text, tb, nt, st.prefix, st.head, ix.start, n_start, s); });
        pin_status[t][0] = INT64_MAX; pin_status[t][1] = 0; pin_status[t][2] = 0; pin_status[t][3] = 0;
        q.up(st.status, pin_status[t], 4 * sizeof(int64_t));
        q.run(MPB_K_FQ_ROWS, [&] { mpb_launch_fq_rows(st.text, tb, ix.start, n_start, count, 0, ix.idx, ix.kinds, ix.desc, st.status, s); });
        q.down(pin_status[t], st.status, 4 * sizeof(int64_t));
    }
    MpbLdsClasses classes{};
    classes.n = k_n_class;
    for (int k = 0; k < k_n_class; k++) classes.cap[k] = k_lds_class[k];
    pst[0] = INT64_MAX; pst[1] = INT64_MAX; pst[2] = 0; pst[3] = 0;
    if (m > 0) {
        q.up(ps.status, pst, 4 * sizeof(int64_t));
        q.run(MPB_K_CONTIG_ROWS, [&] {
            mpb_launch_pair_rows(in[0].ix.idx, in[1].ix.idx, m, in[0].st.text, bytes[0], in[1].st.text, bytes[1], (int)maxabs, !whole_back,
                                 classes, ps.rows, ps.cls, ps.status, s); });
        q.down(pst, ps.status, 4 * sizeof(int64_t));
    }
    if (q.pending && (rc = q.wait("k_fq_starts / k_fq_rows / k_pair_rows"))) return rc;
    // 4. the counts of the call
    for (int t = 0; t < 2; t++)
        if (!index_verdict(pin_status[t], cand[t], in[t])) { *why = MPB_FQ_WHY_ROW_CHECK; *which = t; return MPB_OK; }
    const int64_t np = std::min(in[0].n, in[1].n);
    const int64_t mis = pst[0] < np ? pst[0] : -1;
    const int64_t nb = mis < 0 ? np : mis;
    if (pst[1] < nb) { *why = MPB_FQ_WHY_ROW_CHECK; *which = 0; return MPB_OK; }
    // the rows of both indexes, the offenders' kinds and the two bytes behind pair n_pairs - 1, for the caller's arrays
    uint32_t *const consumed32[2] = {&pin_head[0][0], &pin_head[1][0]};
    uint8_t *const kind8[2] = {(uint8_t *)&pin_head[0][1], (uint8_t *)&pin_head[1][1]};
    int64_t *const idx_out[2] = {fidx_out, ridx_out};
    for (int t = 0; t < 2; t++) { *consumed32[t] = 0; *kind8[t] = 0; }
    auto index_out = [&](StreamQueue &qq) {
        for (int t = 0; t < 2; t++) {
            qq.down(idx_out[t], in[t].ix.idx, in[t].rows * MPB_IDX_COLS * (int64_t)sizeof(int64_t));
            if (np > 0) qq.down(consumed32[t], in[t].ix.start + 4 * np, sizeof(uint32_t));
            if (in[t].rows > in[t].n) qq.down(kind8[t], in[t].ix.kinds + in[t].n, 1);
        }
    };
    auto counts_out = [&] {
        *n_f = in[0].n; *n_r = in[1].n; *f_bad_kind = (int32_t)*kind8[0]; *r_bad_kind = (int32_t)*kind8[1];
        *n_pairs = np; *mismatch = mis; *n_built = nb; *f_consumed = (int64_t)*consumed32[0]; *r_consumed = (int64_t)*consumed32[1];
    };
    auto index_only = [&]() -> int {
        index_out(q);
        if (q.pending && (rc = q.wait("hipMemcpyAsync (index)"))) return rc;
        counts_out();
        return MPB_OK;
    };
    if (nb == 0) return index_only();
    // 5. the classes' counts and their prefix; one small read-back: the class totals, rec_cap, the longest l1 + l2
    q.run(MPB_K_CONTIG_ROWS, [&] { mpb_launch_pair_count(ps.rows, ps.cls, nb, ps.table, ps.prefix, ps.head, ps.status, s); });
    q.down(pst, ps.status, 4 * sizeof(int64_t));
    q.down(c->pin->pair_head, ps.head, MPB_PAIR_HEAD_WORDS * sizeof(uint32_t));
    if ((rc = q.wait("k_pair_count / k_pair_scan"))) return rc;
    const int64_t rec_cap = pst[2] + 8;
    *rec_cap_out = rec_cap;
    if (pst[2] < 0 || rec_cap > out_cap_bytes / nb) {
        *n_pairs = np;
        return fail(MPB_E_INVALID, "out_cap_bytes %lld is too small: %lld pairs of rec_cap %lld", (long long)out_cap_bytes, (long long)nb,
                    (long long)rec_cap);
    }
    ContigWork w{};
    int64_t listed = 0;
    for (int k = 0; k < k_n_class; k++) { w.per_class[k] = c->pin->pair_head[k]; w.first[k] = listed; listed += w.per_class[k]; }
    if (listed > nb || pst[3] < 0 || pst[3] > 2 * MPB_CONTIG_MAX_LEN) { *why = MPB_FQ_WHY_ROW_CHECK; return MPB_OK; }
    memset(filtered, 0, (size_t)nb);
    if (listed == 0) {
        memset(done, 0, (size_t)nb);
        if (n_handed_back) *n_handed_back = nb;
        return index_only();
    }
    if (params->consensus == 2 && (rc = ensure_tables(c))) return rc;
    // 6. the lists, then the chunk call from its step 4 on; the contig stage holds no second copy of the texts
    w.longest = pst[3];
    ContigStage st{};
    TextStage ts{};
    int64_t stride = 0, piece_rows = 0;
    if ((rc = contig_blocks(c, st, ts, 0, 0, 0, nb, rec_cap, 0, w.longest, &fa, &stride, &piece_rows))) return rc;
    q.zero(st.done, nb);
    q.run(MPB_K_CONTIG_ROWS, [&] { mpb_launch_pair_lists(ps.cls, nb, ps.prefix, ps.head, ps.list, s); });
    w.ftext = in[0].st.text; w.fbytes = bytes[0]; w.rtext = in[1].st.text; w.rbytes = bytes[1]; w.rows = ps.rows; w.list = ps.list;
    rc = contigs_run(q, w, st, ts, stride, piece_rows, nb, fastq_offset, params, maxabs, rec_cap, out_buf, out_idx, overlap, gaps,
                     mismatches, done, nullptr, 0, nullptr, nullptr, n_done, n_handed_back, &fa, fres, index_out);
    if (rc) return rc;
    counts_out();
    // 7. every pair built and filtered on the device: the slots, their index and the three arrays stay where they lie, the resident
    // text of a new generation (all or nothing: a handed-back pair or a refused filter leaves none)
    if (*why == MPB_FQ_WHY_TAKEN && nb > 0 && *n_handed_back == 0 && *filter_rc == MPB_OK)
        resident_keep_contigs(c, st.out_buf, nb * rec_cap, st.out_idx, nb, st.overlap, st.gaps, st.mism);
    return MPB_OK;
}
