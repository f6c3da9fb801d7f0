// mpb_fasta_qual.cpp -- fasta+qual input on the device, behind the C ABI of libmoira_pb.so (include/moira_pb.h): the entry that
// takes a chunk of fasta text and a chunk of qual text and returns mio_fasta_qual_index's buffer and index
// (mpb_fasta_qual_index_host), and the one that filters the records from the same upload and leaves buffer and index on the
// device as the resident text of a new generation (mpb_filter_fasta_qual_host: the device-written descriptors go straight into
// mpb_text.cpp's piece loop).  Both texts go through the FASTQ index's line kernels (mpb_index_kernels.hip); the record stage is
// mpb_fasta_qual_kernels.hip.  Texts the device does not take are handed back with a reason.  Each entry queues on one
// StreamQueue (mpb_queue.h); the blocks are the FASTQ index's two (c->fastq_stage, c->fastq_index).
// (Every mpb_* function defined here has C linkage: include/moira_pb.h declares it inside extern "C".)

#include "mpb_ctx.h"

#include <cstring>

namespace {

struct FaAsk {
    const char *ftext; int64_t fbytes; const char *qtext; int64_t qbytes; int32_t final; int64_t max_records; int32_t max_len;
    int64_t out_cap, idx_cap_rows;
};

// what the device made of two texts it took: everything lies in c->fastq_stage (texts, out) and c->fastq_index (the rest)
struct FaIndexed {
    FastqStage f{}, q{};
    uint8_t *out = nullptr; int64_t out_bytes = 0;           // the slots; its allocation
    uint32_t *fstart = nullptr, *qstart = nullptr;
    int64_t *size = nullptr, *prefix = nullptr, *head = nullptr, *idx = nullptr; mpb_text_row *desc = nullptr;
    int64_t n = 0, out_used = 0, longest = 0;
    void layout_index(Carver &k, int64_t n_start, int64_t rows)
    {
        k.take(fstart, n_start); k.take(qstart, n_start);
        k.take(size, rows); k.take(prefix, rows + 1); k.take(head, 4);
        k.take(idx, rows * MPB_IDX_COLS); k.take(desc, rows);
    }
};

int check_args(const FaAsk &a, bool out_needed, const void *out, const int64_t *idx_out, const int64_t *n, const int64_t *f_consumed,
               const int64_t *q_consumed, const int64_t *out_used, const int32_t *why, const int32_t *which, const int64_t *bad_record,
               const char *who)
{
    if (a.fbytes < 0 || a.qbytes < 0 || (a.fbytes > 0 && !a.ftext) || (a.qbytes > 0 && !a.qtext) || a.max_records < 0 || a.max_len < 0 || a.out_cap < 0 ||
        a.idx_cap_rows < 0 || (out_needed && !out) || !idx_out || !n || !f_consumed || !q_consumed || !out_used || !why || !which ||
        !bad_record)
        return fail(MPB_E_INVALID, "%s: bad arguments", who);
    if (a.out_cap > k_text_max_bytes)
        return fail(MPB_E_INVALID, "%s: out_cap %lld exceeds 1 GiB; split the chunk", who, (long long)a.out_cap);
    int rc = check_text_bytes(a.fbytes);
    return rc ? rc : check_text_bytes(a.qbytes);
}

// Uploads, the line kernels over both texts, the record stage and the two small read-backs.  *why != 0: handed back.
// *n_needed: the candidate records, once the lines are counted.
int index_on_device(StreamQueue &q, const FaAsk &a, int64_t *n_needed, FaIndexed &o, int32_t *why, int32_t *which, int64_t *bad_record)
{
    *why = MPB_FQ_WHY_TAKEN; *which = 0; *bad_record = -1;
    mpb_ctx *c = q.c;
    hipStream_t s = c->stream;
    const int64_t f_tiles = (a.fbytes + MPB_FQ_TILE - 1) / MPB_FQ_TILE, q_tiles = (a.qbytes + MPB_FQ_TILE - 1) / MPB_FQ_TILE;
    // a slot is a header token and twice a sequence of the fasta text: the slots of all records are at most twice that text
    o.out_bytes = a.out_cap < 2 * a.fbytes ? a.out_cap : 2 * a.fbytes;
    int rc;
    if ((rc = carve(c, c->fastq_stage, [&](Carver &k) {
            o.f.layout(k, a.fbytes, f_tiles); o.q.layout(k, a.qbytes, q_tiles); k.take(o.out, align_up(o.out_bytes > 0 ? o.out_bytes : 1, 16)); })))
        return rc;
    q.up(o.f.text, a.ftext, a.fbytes);
    q.up(o.q.text, a.qtext, a.qbytes);
    q.run(MPB_K_FQ_LINES, [&] {
        mpb_launch_fq_lines(o.f.text, a.fbytes, f_tiles, o.f.info, s);
        mpb_launch_fq_lines(o.q.text, a.qbytes, q_tiles, o.q.info, s); });
    q.run(MPB_K_FQ_SCAN, [&] {
        mpb_launch_fq_scan(o.f.text, a.fbytes, a.final != 0, o.f.info, f_tiles, o.f.prefix, o.f.head, s);
        mpb_launch_fq_scan(o.q.text, a.qbytes, a.final != 0, o.q.info, q_tiles, o.q.prefix, o.q.head, s); });
    const uint32_t *head[2] = {c->pin->fq_head, c->pin->fq_head2};
    q.down(c->pin->fq_head, o.f.head, 4 * sizeof(uint32_t));
    q.down(c->pin->fq_head2, o.q.head, 4 * sizeof(uint32_t));
    if ((rc = q.wait("hipMemcpyAsync (text upload) / k_fq_lines / k_fq_scan"))) return rc;
    for (int t = 0; t < 2; t++) {
        if (head[t][1] & 2u) { *why = MPB_FQ_WHY_LONE_CR; *which = t; return MPB_OK; }
        if (head[t][1] & 1u) { *why = MPB_FQ_WHY_NON_ASCII; *which = t; return MPB_OK; }
    }
    // the counted lines size the rest
    const int64_t lines[2] = {head[0][2], head[1][2]};
    int64_t cand = a.max_records;
    for (int t = 0; t < 2; t++) if (lines[t] / 2 < cand) cand = lines[t] / 2;
    // at the end of the files anything but "both exhausted" is the line parser's business (the host: !(fp >= flen && qp >= qlen))
    if (a.final && cand < a.max_records && (lines[0] > 2 * cand || lines[1] > 2 * cand)) {
        *why = MPB_FA_WHY_TRUNCATED; *which = lines[0] > 2 * cand ? 0 : 1;
        return MPB_OK;
    }
    *n_needed = cand;
    if (cand > a.idx_cap_rows)
        return fail(MPB_E_INVALID, "idx_cap_rows %lld is too small: the texts hold %lld records", (long long)a.idx_cap_rows, (long long)cand);
    const int64_t n_start = 2 * cand + 1;
    Carver size;
    o.layout_index(size, n_start, cand > 0 ? cand : 1);
    if (size.bytes() > MPB_FQ_INDEX_MAX_BYTES) { *why = MPB_FQ_WHY_LINE_TABLE; return MPB_OK; }
    rc = carve(c, c->fastq_index, [&](Carver &k) { o.layout_index(k, n_start, cand > 0 ? cand : 1); });
    if (rc == MPB_E_NOMEM) { *why = MPB_FQ_WHY_LINE_TABLE; return MPB_OK; }
    if (rc) return rc;
    if (cand == 0) return MPB_OK;                            // (n = 0, nothing consumed, nothing used)
    int64_t *status = c->pin->fq_status, *scan = c->pin->fq_status2;
    status[0] = INT64_MAX; status[1] = 0; status[2] = 0; status[3] = 0;
    q.up(o.f.status, status, 4 * sizeof(int64_t));
    q.run(MPB_K_FQ_STARTS, [&] {
        mpb_launch_fq_starts(o.f.text, a.fbytes, f_tiles, o.f.prefix, o.f.head, o.fstart, n_start, s);
        mpb_launch_fq_starts(o.q.text, a.qbytes, q_tiles, o.q.prefix, o.q.head, o.qstart, n_start, s); });
    q.run(MPB_K_FQ_ROWS, [&] {
        mpb_launch_fa_count(o.f.text, a.fbytes, o.fstart, o.q.text, a.qbytes, o.qstart, n_start, cand, a.out_cap, o.size, o.prefix, o.head,
                            o.f.status, s);
        mpb_launch_fa_write(o.f.text, a.fbytes, o.fstart, o.q.text, a.qbytes, o.qstart, n_start, cand, a.max_len, o.prefix, o.head, o.out,
                            o.out_bytes, o.idx, o.desc, o.f.status, s); });
    q.down(status, o.f.status, 4 * sizeof(int64_t));
    q.down(scan, o.head, 4 * sizeof(int64_t));
    if ((rc = q.wait("k_fq_starts / k_fa_count / k_fa_scan / k_fa_write"))) return rc;
    if (status[0] != INT64_MAX) {
        const int64_t rec = status[0] >> 8;
        const int32_t w = (int32_t)((status[0] >> 1) & 127);
        if (status[0] < 0 || rec >= cand || w < MPB_FQ_WHY_ROW_CHECK || w > MPB_FA_WHY_LENGTH) { *why = MPB_FQ_WHY_ROW_CHECK; return MPB_OK; }
        *why = w; *which = (int32_t)(status[0] & 1); *bad_record = rec;
        return MPB_OK;
    }
    if (status[2] != 0 || scan[0] < 0 || scan[0] > cand || scan[1] < 0 || scan[1] > o.out_bytes || status[1] < 0 ||
        status[1] > k_text_max_bytes) {
        *why = MPB_FQ_WHY_ROW_CHECK;
        return MPB_OK;
    }
    o.n = scan[0]; o.out_used = scan[1]; o.longest = status[1];
    return MPB_OK;
}

// the rows of the index, the slots and the first bytes behind the last record of either text, queued for the caller's arrays
void queue_out(StreamQueue &q, const FaIndexed &in, uint8_t *out, int64_t *idx_out, uint32_t *consumed32)
{
    q.down(idx_out, in.idx, in.n * MPB_IDX_COLS * (int64_t)sizeof(int64_t));
    if (out) q.down(out, in.out, in.out_used);
    if (in.n > 0) {
        q.down(consumed32 + 0, in.fstart + 2 * in.n, sizeof(uint32_t));
        q.down(consumed32 + 1, in.qstart + 2 * in.n, sizeof(uint32_t));
    }
}

}  // namespace

int mpb_fasta_qual_index_host(mpb_ctx *c, const char *ftext, int64_t ftext_bytes, const char *qtext, int64_t qtext_bytes, int32_t final,
                              int64_t max_records, int32_t max_len, uint8_t *out, int64_t out_cap, int64_t *idx_out, int64_t idx_cap_rows,
                              int64_t *n, int64_t *f_consumed, int64_t *q_consumed, int64_t *out_used, int32_t *why, int32_t *which,
                              int64_t *bad_record)
{
    // (the arguments first: what is wrong with them is said with or without a device)
    const FaAsk a{ftext, ftext_bytes, qtext, qtext_bytes, final, max_records, max_len, out_cap, idx_cap_rows};
    int rc = check_args(a, true, out, idx_out, n, f_consumed, q_consumed, out_used, why, which, bad_record, "mpb_fasta_qual_index_host");
    if (rc) return rc;
    CTXCHK(c);
    resident_drop(c);
    *n = 0; *f_consumed = 0; *q_consumed = 0; *out_used = 0;
    FaIndexed in;
    StreamQueue q(c);
    if ((rc = index_on_device(q, a, n, in, why, which, bad_record))) return rc;
    *n = 0;
    if (*why) return MPB_OK;
    // (the two small words land in the pinned block: nothing of them lies on a frame)
    uint32_t *consumed32 = &c->pin->fq_head[0];
    consumed32[0] = 0; consumed32[1] = 0;
    queue_out(q, in, out, idx_out, consumed32);
    if ((rc = q.wait("hipMemcpyAsync (index, slots)"))) return rc;
    *n = in.n; *f_consumed = (int64_t)consumed32[0]; *q_consumed = (int64_t)consumed32[1]; *out_used = in.out_used;
    return MPB_OK;
}

int mpb_filter_fasta_qual_host(mpb_ctx *c, const char *ftext, int64_t ftext_bytes, const char *qtext, int64_t qtext_bytes, int32_t final,
                               int64_t max_records, int32_t max_len, uint8_t *out, int64_t out_cap, int64_t *idx_out,
                               int64_t idx_cap_rows, int64_t *n, int64_t *f_consumed, int64_t *q_consumed, int64_t *out_used,
                               int32_t *why, int32_t *which, int64_t *bad_record, int32_t lower_n_is_base,
                               const mpb_filter_params *params, int32_t poisson, double *ee, int32_t *ns, uint8_t *pass,
                               int32_t *len_out, uint8_t *flags_out, mpb_filter_counts *counts, int64_t *bad_pack_record)
{
    if (bad_pack_record) *bad_pack_record = -1;
    int rc = check_params(params);
    if (rc) return rc;
    const FaAsk a{ftext, ftext_bytes, qtext, qtext_bytes, final, max_records, max_len, out_cap, idx_cap_rows};
    if ((rc = check_args(a, false, out, idx_out, n, f_consumed, q_consumed, out_used, why, which, bad_record, "mpb_filter_fasta_qual_host")))
        return rc;
    if (!ee || !ns || !pass) return fail(MPB_E_INVALID, "NULL host buffer");
    CTXCHK(c);
    resident_drop(c);
    *n = 0; *f_consumed = 0; *q_consumed = 0; *out_used = 0;
    if (counts) memset(counts, 0, sizeof(*counts));
    FaIndexed in;
    TextResults res{ee, ns, pass, len_out, flags_out, {}};
    StreamQueue q(c);
    if ((rc = index_on_device(q, a, n, in, why, which, bad_record))) return rc;
    *n = 0;
    if (*why) return MPB_OK;
    if (in.n > 0x7fffffffll - 4096) return fail(MPB_E_INVALID, "batch of %lld reads exceeds 2^31; split it", (long long)in.n);
    if (in.longest > MPB_MAX_LEN)
        return fail(MPB_E_INVALID, "reads longer than 65535 bases are not supported; length (%lld)", (long long)in.longest);
    int64_t n_pass = 0, n_overflow = 0;
    TextStage st{};
    if (in.n > 0) {
        // the slots are the text of the filter: its qualities are bytes, so the FASTQ offset is 0
        const int64_t stride = align_up(in.longest > 1 ? in.longest : 1, 128);
        const int64_t piece_rows = text_piece_rows(in.n, stride);
        if ((rc = carve(c, c->text_stage, [&](Carver &k) { st.layout_results(k, in.n, piece_rows, stride); }))) return rc;
        if ((rc = filter_text_pieces(q, in.out, in.out_used, in.desc, in.n, stride, piece_rows, 0, lower_n_is_base, params, poisson, st,
                                     &n_pass, &n_overflow, bad_pack_record))) return rc;
    }
    uint32_t *consumed32 = &c->pin->fq_head[0];
    consumed32[0] = 0; consumed32[1] = 0;
    queue_out(q, in, out, idx_out, consumed32);
    if (in.n > 0) rc = text_results_out(q, st, in.n, params, poisson, res, &n_pass);
    else rc = q.wait("hipMemcpyAsync (index, slots)");
    if (rc) return rc;
    *n = in.n; *f_consumed = (int64_t)consumed32[0]; *q_consumed = (int64_t)consumed32[1]; *out_used = in.out_used;
    // the slots and the device-written index stay where they lie: the resident text of a new generation
    Indexed keep;
    keep.st.text = in.out; keep.ix.idx = in.idx; keep.n = in.n;
    resident_keep(c, keep, in.out_used);
    if (counts) { counts->n_reads = in.n; counts->n_pass = n_pass; counts->n_fail = in.n - n_pass; counts->n_overflow = n_overflow; }
    return MPB_OK;
}
