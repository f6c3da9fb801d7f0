// mpb_index.cpp -- the FASTQ record index on the device, behind the C ABI of libmoira_pb.so (include/moira_pb.h): the entry that
// takes a chunk of FASTQ text alone and returns mio_fastq_index's index (mpb_fastq_index_host), and the one that filters the
// chunk from the same upload (mpb_filter_fastq_host: the index's device-written descriptors go straight into mpb_text.cpp's
// piece loop; filter_indexed, the tail it shares with mpb_bgzf_fastq.cpp).  The kernels are mpb_index_kernels.hip; a text the
// device does not take is handed back with a reason.  Each entry queues on one StreamQueue (mpb_queue.h).
// (Every mpb_* function defined here has C linkage: include/moira_pb.h declares it inside extern "C".)

#include "mpb_ctx.h"

#include <cstring>

namespace {

int check_args(const char *text, int64_t text_bytes, int64_t max_records, int32_t max_len, const int64_t *idx_out, int64_t idx_cap_rows,
               const int64_t *n, const int64_t *consumed, const int32_t *bad_kind, const int32_t *why, const char *who)
{
    if (text_bytes < 0 || (text_bytes > 0 && !text) || max_records < 0 || max_len < 0 || idx_cap_rows < 1 || !idx_out || !n || !consumed ||
        !bad_kind || !why)
        return fail(MPB_E_INVALID, "%s: bad arguments", who);
    return check_text_bytes(text_bytes);
}

}  // namespace

// k_fq_lines, k_fq_scan and the copy of the head words to the pinned block, queued over the text that lies in out.st.text
void fastq_index_queue_head(StreamQueue &q, Indexed &out, int64_t text_bytes, int32_t final, uint32_t *pin_head)
{
    hipStream_t s = q.c->stream;
    const int64_t n_tiles = (text_bytes + MPB_FQ_TILE - 1) / MPB_FQ_TILE;
    FastqStage &st = out.st;
    q.run(MPB_K_FQ_LINES, [&] { mpb_launch_fq_lines(st.text, text_bytes, n_tiles, st.info, s); });
    q.run(MPB_K_FQ_SCAN, [&] { mpb_launch_fq_scan(st.text, text_bytes, final != 0, st.info, n_tiles, st.prefix, st.head, s); });
    q.down(pin_head ? pin_head : q.c->pin->fq_head, st.head, 4 * sizeof(uint32_t));
}

// What follows the wait behind fastq_index_queue_head: the head words' verdict, the blocks sized from the counted lines,
// k_fq_starts, k_fq_rows and its small read-back.  *why != 0: handed back.  The index stays on the device (out.ix).
int fastq_index_finish(StreamQueue &q, int64_t text_bytes, int64_t max_records, int32_t max_len, int64_t idx_cap_rows, int64_t *n_needed,
                       Indexed &out, int32_t *why)
{
    *why = MPB_FQ_WHY_TAKEN;
    mpb_ctx *c = q.c;
    hipStream_t s = c->stream;
    const int64_t n_tiles = (text_bytes + MPB_FQ_TILE - 1) / MPB_FQ_TILE;
    FastqStage &st = out.st;
    const uint32_t *head = c->pin->fq_head;
    int64_t *status = c->pin->fq_status;
    int rc;
    if (head[1] & 2u) { *why = MPB_FQ_WHY_LONE_CR; return MPB_OK; }
    if (head[1] & 1u) { *why = MPB_FQ_WHY_NON_ASCII; return MPB_OK; }
    // the counted lines size the rest
    const int64_t lines = head[2];
    const int64_t cand = lines / 4 < max_records ? lines / 4 : max_records;          // records the text can hold, good or bad
    *n_needed = cand;
    if (cand + 1 > idx_cap_rows)
        return fail(MPB_E_INVALID, "idx_cap_rows %lld is too small: the text holds %lld records, and the row after them may be written",
                    (long long)idx_cap_rows, (long long)cand);
    const int64_t n_start = 4 * cand + 1;
    FastqIndex &ix = out.ix;
    Carver size;
    ix.layout(size, n_start, cand > 0 ? cand : 1);
    if (size.bytes() > MPB_FQ_INDEX_MAX_BYTES) { *why = MPB_FQ_WHY_LINE_TABLE; return MPB_OK; }
    rc = carve(c, c->fastq_index, [&](Carver &k) { ix.layout(k, n_start, cand > 0 ? cand : 1); });
    if (rc == MPB_E_NOMEM) { *why = MPB_FQ_WHY_LINE_TABLE; return MPB_OK; }
    if (rc) return rc;
    if (cand == 0) return MPB_OK;                            // (n = 0, consumed = 0, no bad record)
    q.run(MPB_K_FQ_STARTS, [&] { mpb_launch_fq_starts(st.text, text_bytes, n_tiles, st.prefix, st.head, ix.start, n_start, s); });
    // the rows; when a record fails its checks, once more over the records before it: the longest packed length is theirs alone
    int64_t count = cand;
    for (int pass = 0; pass < 2; pass++) {
        status[0] = INT64_MAX; status[1] = 0; status[2] = 0; status[3] = 0;
        q.up(st.status, status, 4 * sizeof(int64_t));
        q.run(MPB_K_FQ_ROWS, [&] {
            mpb_launch_fq_rows(st.text, text_bytes, ix.start, n_start, count, max_len, ix.idx, ix.kinds, ix.desc, st.status, s); });
        q.down(status, st.status, 4 * sizeof(int64_t));
        if ((rc = q.wait("k_fq_starts / k_fq_rows"))) return rc;
        if (status[2] != 0) { *why = MPB_FQ_WHY_ROW_CHECK; return MPB_OK; }
        if (pass == 1 || status[0] == INT64_MAX) break;
        if (status[0] < 0 || status[0] >= count) { *why = MPB_FQ_WHY_ROW_CHECK; return MPB_OK; }
        count = status[0];                                   // (0: no record before the offender; nothing to look at again)
        out.rows = count + 1;
        if (count == 0) { status[1] = 0; break; }
    }
    out.n = count;
    if (out.rows == 0) out.rows = count;
    out.longest = status[1];
    if (out.longest < 0 || out.longest > k_text_max_bytes) { *why = MPB_FQ_WHY_ROW_CHECK; return MPB_OK; }
    return MPB_OK;
}

namespace {

// Upload, the four kernels and the two small read-backs.  *why != 0: handed back.  The index stays on the device (out.ix).
int index_on_device(StreamQueue &q, const char *text, int64_t text_bytes, int32_t final, int64_t max_records, int32_t max_len,
                    int64_t idx_cap_rows, int64_t *n_needed, Indexed &out, int32_t *why)
{
    *why = MPB_FQ_WHY_TAKEN;
    const int64_t n_tiles = (text_bytes + MPB_FQ_TILE - 1) / MPB_FQ_TILE;
    FastqStage &st = out.st;
    int rc;
    if ((rc = carve(q.c, q.c->fastq_stage, [&](Carver &k) { st.layout(k, text_bytes, n_tiles); }))) return rc;
    q.up(st.text, text, text_bytes);
    fastq_index_queue_head(q, out, text_bytes, final);
    if ((rc = q.wait("hipMemcpyAsync (text upload) / k_fq_lines / k_fq_scan"))) return rc;
    return fastq_index_finish(q, text_bytes, max_records, max_len, idx_cap_rows, n_needed, out, why);
}

}  // namespace

void resident_keep(mpb_ctx *c, const Indexed &in, int64_t text_bytes)
{
    c->resident.gen = ++c->resident.last;
    c->resident.text = in.st.text; c->resident.text_bytes = text_bytes; c->resident.idx = in.ix.idx; c->resident.n = in.n;
    c->resident.in_contig_stage = false;
    c->resident.aux[0] = c->resident.aux[1] = c->resident.aux[2] = nullptr;
}

void resident_keep_contigs(mpb_ctx *c, const uint8_t *slots, int64_t text_bytes, const int64_t *idx, int64_t n, const int32_t *overlap,
                           const int32_t *gaps, const int32_t *mism)
{
    c->resident.gen = ++c->resident.last;
    c->resident.text = slots; c->resident.text_bytes = text_bytes; c->resident.idx = idx; c->resident.n = n;
    c->resident.in_contig_stage = true;
    c->resident.aux[0] = overlap; c->resident.aux[1] = gaps; c->resident.aux[2] = mism;
}

void resident_drop(mpb_ctx *c) { c->resident.gen = 0; }

void resident_drop_contigs(mpb_ctx *c) { if (c->resident.in_contig_stage) c->resident.gen = 0; }

int64_t mpb_resident_text(mpb_ctx *c) { return c ? c->resident.gen : 0; }

// the rows of the index, the offender's kind and the first byte behind the last record, queued for the caller's arrays
void queue_index_out(StreamQueue &q, const Indexed &in, int64_t *idx_out, uint32_t *consumed32, uint8_t *kind8)
{
    q.down(idx_out, in.ix.idx, in.rows * MPB_IDX_COLS * (int64_t)sizeof(int64_t));
    if (in.n > 0) q.down(consumed32, in.ix.start + 4 * in.n, sizeof(uint32_t));
    if (in.rows > in.n) q.down(kind8, in.ix.kinds + in.n, 1);
}

int filter_indexed(StreamQueue &q, const Indexed &in, int64_t text_bytes, uint8_t *text_out, int64_t *idx_out, int64_t *n,
                   int64_t *consumed, int32_t *bad_kind, const FastqFilterAsk &ask, TextResults &r)
{
    mpb_ctx *c = q.c;
    int rc;
    if (in.n > 0x7fffffffll - 4096) return fail(MPB_E_INVALID, "batch of %lld reads exceeds 2^31; split it", (long long)in.n);
    if (in.longest > MPB_MAX_LEN)
        return fail(MPB_E_INVALID, "reads longer than 65535 bases are not supported; length (%lld)", (long long)in.longest);
    int64_t n_pass = 0, n_overflow = 0;
    TextStage st{};
    if (in.n > 0) {
        const int64_t stride = align_up(in.longest > 1 ? in.longest : 1, 128);
        const int64_t piece_rows = text_piece_rows(in.n, stride);
        if ((rc = carve(c, c->text_stage, [&](Carver &k) { st.layout_results(k, in.n, piece_rows, stride); }))) return rc;
        if ((rc = filter_text_pieces(q, in.st.text, text_bytes, in.ix.desc, in.n, stride, piece_rows, ask.fastq_offset, ask.lower_n_is_base,
                                     ask.params, ask.poisson, st, &n_pass, &n_overflow, ask.bad_record))) return rc;
    }
    // (the two small words land in the pinned block: nothing of them lies on a frame)
    uint32_t *consumed32 = &c->pin->fq_head[0];
    uint8_t *kind8 = (uint8_t *)&c->pin->fq_head[1];
    *consumed32 = 0; *kind8 = 0;
    queue_index_out(q, in, idx_out, consumed32, kind8);
    if (text_out) q.down(text_out, in.st.text, text_bytes);
    if (in.n > 0) rc = text_results_out(q, st, in.n, ask.params, ask.poisson, r, &n_pass);
    else rc = q.wait("hipMemcpyAsync (index, text)");
    if (rc) return rc;
    *n = in.n; *consumed = (int64_t)*consumed32; *bad_kind = (int32_t)*kind8;
    resident_keep(c, in, text_bytes);
    if (ask.counts) { ask.counts->n_reads = in.n; ask.counts->n_pass = n_pass; ask.counts->n_fail = in.n - n_pass; ask.counts->n_overflow = n_overflow; }
    return MPB_OK;
}

int mpb_fastq_index_host(mpb_ctx *c, const char *text, int64_t text_bytes, int32_t final, int64_t max_records, int32_t max_len,
                         int64_t *idx_out, int64_t idx_cap_rows, int64_t *n, int64_t *consumed, int32_t *bad_kind, int32_t *why)
{
    // (the arguments first: what is wrong with them is said with or without a device)
    int rc = check_args(text, text_bytes, max_records, max_len, idx_out, idx_cap_rows, n, consumed, bad_kind, why, "mpb_fastq_index_host");
    if (rc) return rc;
    CTXCHK(c);
    resident_drop(c);
    *n = 0; *consumed = 0; *bad_kind = 0;
    Indexed in;
    StreamQueue q(c);
    if ((rc = index_on_device(q, text, text_bytes, final, max_records, max_len, idx_cap_rows, n, in, why))) return rc;
    *n = 0;
    if (*why) return MPB_OK;
    // (the two small words land in the pinned block: nothing of them lies on a frame)
    uint32_t *consumed32 = &c->pin->fq_head[0];
    uint8_t *kind8 = (uint8_t *)&c->pin->fq_head[1];
    *consumed32 = 0; *kind8 = 0;
    queue_index_out(q, in, idx_out, consumed32, kind8);
    if ((rc = q.wait("hipMemcpyAsync (index)"))) return rc;
    *n = in.n; *consumed = (int64_t)*consumed32; *bad_kind = (int32_t)*kind8;
    return MPB_OK;
}

int mpb_filter_fastq_host(mpb_ctx *c, const char *text, int64_t text_bytes, int32_t final, int64_t max_records, int32_t max_len,
                          int64_t *idx_out, int64_t idx_cap_rows, int64_t *n, int64_t *consumed, int32_t *bad_kind, int32_t *why,
                          int32_t fastq_offset, int32_t lower_n_is_base, const mpb_filter_params *params, int32_t poisson,
                          double *ee, int32_t *ns, uint8_t *pass, int32_t *len_out, uint8_t *flags_out,
                          mpb_filter_counts *counts, int64_t *bad_record)
{
    if (bad_record) *bad_record = -1;
    int rc = check_params(params);
    if (rc) return rc;
    if ((rc = check_args(text, text_bytes, max_records, max_len, idx_out, idx_cap_rows, n, consumed, bad_kind, why, "mpb_filter_fastq_host")))
        return rc;
    if (!ee || !ns || !pass) return fail(MPB_E_INVALID, "NULL host buffer");
    if ((rc = check_fastq_offset(fastq_offset))) return rc;
    CTXCHK(c);
    resident_drop(c);
    *n = 0; *consumed = 0; *bad_kind = 0;
    if (counts) memset(counts, 0, sizeof(*counts));
    Indexed in;
    TextResults res{ee, ns, pass, len_out, flags_out, {}};
    StreamQueue q(c);
    if ((rc = index_on_device(q, text, text_bytes, final, max_records, max_len, idx_cap_rows, n, in, why))) return rc;
    *n = 0;
    if (*why) return MPB_OK;
    return filter_indexed(q, in, text_bytes, nullptr, idx_out, n, consumed, bad_kind,
                          FastqFilterAsk{fastq_offset, lower_n_is_base, params, poisson, counts, bad_record}, res);
}
