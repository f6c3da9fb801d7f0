// mpb_index.cpp -- the FASTQ record index on the device, behind the C ABI of libmoira_pb.so (include/moira_pb.h): the entry that
// takes a chunk of FASTQ text alone and returns mio_fastq_index's index (mpb_fastq_index_host), and the one that filters the
// chunk from the same upload (mpb_filter_fastq_host: the index's device-written descriptors go straight into mpb_text.cpp's
// piece loop).  The kernels are mpb_index_kernels.hip; a text the device does not take is handed back with a reason.
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
    if (text_bytes > k_text_max_bytes)
        return fail(MPB_E_INVALID, "text of %lld bytes: one call takes at most %lld bytes (1 GiB) of text; split the chunk",
                    (long long)text_bytes, (long long)k_text_max_bytes);
    return MPB_OK;
}

}  // namespace

// k_fq_lines, k_fq_scan and the copy of the head words to the pinned block, queued over the text that lies in out.st.text
hipError_t fastq_index_queue_head(mpb_ctx *c, Indexed &out, int64_t text_bytes, int32_t final)
{
    hipStream_t s = c->stream;
    const int64_t n_tiles = (text_bytes + MPB_FQ_TILE - 1) / MPB_FQ_TILE;
    FastqStage &st = out.st;
    { Span t(c, MPB_K_FQ_LINES); mpb_launch_fq_lines(st.text, text_bytes, n_tiles, st.info, s); }
    { Span t(c, MPB_K_FQ_SCAN); mpb_launch_fq_scan(st.text, text_bytes, final != 0, st.info, n_tiles, st.prefix, st.head, s); }
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(c->pin->fq_head, st.head, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, s);
    return e;
}

// What follows the synchronisation behind fastq_index_queue_head: the head words' verdict, the blocks sized from the counted
// lines, k_fq_starts, k_fq_rows and its small read-back.  *why != 0: handed back.  The index stays on the device (out.ix); the
// stream is synchronised when this returns, whatever it returns.
int fastq_index_finish(mpb_ctx *c, int64_t text_bytes, int64_t max_records, int32_t max_len, int64_t idx_cap_rows, int64_t *n_needed,
                       Indexed &out, int32_t *why)
{
    *why = MPB_FQ_WHY_TAKEN;
    hipStream_t s = c->stream;
    const int64_t n_tiles = (text_bytes + MPB_FQ_TILE - 1) / MPB_FQ_TILE;
    FastqStage &st = out.st;
    const uint32_t *head = c->pin->fq_head;
    int64_t *status = c->pin->fq_status;
    hipError_t e = hipSuccess, e_sync = hipSuccess;
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
    { Span t(c, MPB_K_FQ_STARTS); mpb_launch_fq_starts(st.text, text_bytes, n_tiles, st.prefix, st.head, ix.start, n_start, s); }
    // the rows; when a record fails its checks, once more over the records before it: the longest packed length is theirs alone
    int64_t count = cand;
    for (int pass = 0; pass < 2; pass++) {
        status[0] = INT64_MAX; status[1] = 0; status[2] = 0; status[3] = 0;
        e = hipMemcpyAsync(st.status, status, 4 * sizeof(int64_t), hipMemcpyHostToDevice, s);
        if (e == hipSuccess) {
            { Span t(c, MPB_K_FQ_ROWS);
              mpb_launch_fq_rows(st.text, text_bytes, ix.start, n_start, count, max_len, ix.idx, ix.kinds, ix.desc, st.status, s); }
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(status, st.status, 4 * sizeof(int64_t), hipMemcpyDeviceToHost, s);
        e_sync = hipStreamSynchronize(s);
        HIPCHK_KEPT("k_fq_starts / k_fq_rows", e);
        HIPCHK_KEPT("hipStreamSynchronize", e_sync);
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

// Upload, the four kernels and the two small read-backs.  *why != 0: handed back.  The index stays on the device (out.ix); the
// stream is synchronised when this returns, whatever it returns.
int index_on_device(mpb_ctx *c, const char *text, int64_t text_bytes, int32_t final, int64_t max_records, int32_t max_len,
                    int64_t idx_cap_rows, int64_t *n_needed, Indexed &out, int32_t *why)
{
    *why = MPB_FQ_WHY_TAKEN;
    hipStream_t s = c->stream;
    const int64_t n_tiles = (text_bytes + MPB_FQ_TILE - 1) / MPB_FQ_TILE;
    FastqStage &st = out.st;
    int rc;
    if ((rc = carve(c, c->fastq_stage, [&](Carver &k) { st.layout(k, text_bytes, n_tiles); }))) return rc;
    // (everything below is queued on one stream; the host blocks it reads from -- the caller's text, the pinned words -- outlive
    // the synchronisation that every path out of here passes)
    hipError_t e = hipSuccess;
    if (text_bytes > 0) e = hipMemcpyAsync(st.text, text, (size_t)text_bytes, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) { (void)hipStreamSynchronize(s); return hip_fail("hipMemcpyAsync (text upload)", e); }
    e = fastq_index_queue_head(c, out, text_bytes, final);
    const hipError_t e_sync = hipStreamSynchronize(s);
    HIPCHK_KEPT("k_fq_lines / k_fq_scan", e);
    HIPCHK_KEPT("hipStreamSynchronize", e_sync);
    return fastq_index_finish(c, text_bytes, max_records, max_len, idx_cap_rows, n_needed, out, why);
}

}  // namespace

// the rows of the index, the offender's kind and the first byte behind the last record, queued for the caller's arrays
hipError_t queue_index_out(mpb_ctx *c, const Indexed &in, int64_t *idx_out, uint32_t *consumed32, uint8_t *kind8)
{
    hipStream_t s = c->stream;
    hipError_t e = hipSuccess;
    if (in.rows > 0) e = hipMemcpyAsync(idx_out, in.ix.idx, (size_t)in.rows * MPB_IDX_COLS * sizeof(int64_t), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && in.n > 0) e = hipMemcpyAsync(consumed32, in.ix.start + 4 * in.n, sizeof(uint32_t), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && in.rows > in.n) e = hipMemcpyAsync(kind8, in.ix.kinds + in.n, 1, hipMemcpyDeviceToHost, s);
    return e;
}

int mpb_fastq_index_host(mpb_ctx *c, const char *text, int64_t text_bytes, int32_t final, int64_t max_records, int32_t max_len,
                         int64_t *idx_out, int64_t idx_cap_rows, int64_t *n, int64_t *consumed, int32_t *bad_kind, int32_t *why)
{
    // (the arguments first: what is wrong with them is said with or without a device)
    int rc = check_args(text, text_bytes, max_records, max_len, idx_out, idx_cap_rows, n, consumed, bad_kind, why, "mpb_fastq_index_host");
    if (rc) return rc;
    CTXCHK(c);
    *n = 0; *consumed = 0; *bad_kind = 0;
    Indexed in;
    if ((rc = index_on_device(c, text, text_bytes, final, max_records, max_len, idx_cap_rows, n, in, why))) return rc;
    *n = 0;
    if (*why) return MPB_OK;
    // (the two small words land in the pinned block: nothing of them lies on a frame)
    uint32_t *consumed32 = &c->pin->fq_head[0];
    uint8_t *kind8 = (uint8_t *)&c->pin->fq_head[1];
    *consumed32 = 0; *kind8 = 0;
    const hipError_t e = queue_index_out(c, in, idx_out, consumed32, kind8);
    const hipError_t e_sync = hipStreamSynchronize(c->stream);
    HIPCHK_KEPT("hipMemcpyAsync (index)", e);
    HIPCHK_KEPT("hipStreamSynchronize", e_sync);
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
    if (fastq_offset < 0 || fastq_offset > 255)
        return fail(MPB_E_INVALID, "fastq_offset %d: the device pack takes offsets 0..255 (beyond them no character is a quality)", fastq_offset);
    CTXCHK(c);
    *n = 0; *consumed = 0; *bad_kind = 0;
    if (counts) memset(counts, 0, sizeof(*counts));
    Indexed in;
    if ((rc = index_on_device(c, text, text_bytes, final, max_records, max_len, idx_cap_rows, n, in, why))) return rc;
    *n = 0;
    if (*why) return MPB_OK;
    if (in.n > 0x7fffffffll - 4096) return fail(MPB_E_INVALID, "batch of %lld reads exceeds 2^31; split it", (long long)in.n);
    if (in.longest > MPB_MAX_LEN)
        return fail(MPB_E_INVALID, "reads longer than 65535 bases are not supported; length (%lld)", (long long)in.longest);
    int64_t n_pass = 0, n_overflow = 0;
    TextStage st{};
    if (in.n > 0) {
        const int64_t stride = align_up(in.longest > 1 ? in.longest : 1, 128);
        const int64_t piece_rows = text_piece_rows(in.n, stride);
        if ((rc = carve(c, c->text_stage, [&](Carver &k) { st.layout_results(k, in.n, piece_rows, stride); }))) return rc;
        if ((rc = filter_text_pieces(c, in.st.text, text_bytes, in.ix.desc, in.n, stride, piece_rows, fastq_offset, lower_n_is_base, params,
                                     poisson, st, &n_pass, &n_overflow, bad_record))) return rc;
    }
    uint32_t *consumed32 = &c->pin->fq_head[0];
    uint8_t *kind8 = (uint8_t *)&c->pin->fq_head[1];
    *consumed32 = 0; *kind8 = 0;
    const hipError_t e = queue_index_out(c, in, idx_out, consumed32, kind8);
    if (e != hipSuccess) { (void)hipStreamSynchronize(c->stream); return hip_fail("hipMemcpyAsync (index)", e); }
    if (in.n > 0) {
        if ((rc = text_results_out(c, st, in.n, params, poisson, ee, ns, pass, len_out, flags_out, &n_pass))) return rc;
    } else {
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    *n = in.n; *consumed = (int64_t)*consumed32; *bad_kind = (int32_t)*kind8;
    if (counts) { counts->n_reads = in.n; counts->n_pass = n_pass; counts->n_fail = in.n - n_pass; counts->n_overflow = n_overflow; }
    return MPB_OK;
}
