// mpb_text.cpp -- FASTQ text as it lies in the file, behind the C ABI of libmoira_pb.so (include/moira_pb.h): the device pack
// from a text buffer and its validated row descriptors (k_pack_text), and the host entry that uploads a chunk's text once,
// packs it on the device and filters it there.  The descriptors come from mpb_text_rows (mpb_hostonly.cpp).  The piece loop
// (filter_text_pieces) takes a text and descriptors that are on the device already: mpb_contig.cpp runs it over contig slots,
// mpb_index.cpp over an indexed text.  The host entry and its helpers queue on one StreamQueue (mpb_queue.h), the caller's.
// (Every mpb_* function defined here has C linkage: include/moira_pb.h declares it inside extern "C".)

#include "mpb_ctx.h"

#include <cstring>
#include <vector>

#define MPB_TEXT_PIECE_BYTES (256ll << 20)   // the piece of the matrix that is packed and filtered at a time

// k0: the position of d_rows[0] in the caller's batch -- the status holds positions counted from it (a batch packed in pieces)
static int pack_text_rows(mpb_ctx *c, const uint8_t *d_text, int64_t text_bytes, const mpb_text_row *d_rows, int64_t n, int64_t k0,
                          int32_t fastq_offset, int32_t lower_n_is_base, int64_t row_stride, uint8_t *d_q_out,
                          int32_t *d_len_out, uint8_t *d_flags_out, int64_t *d_status)
{
    CTXCHK(c);
    if (n < 0 || text_bytes < 0) return fail(MPB_E_INVALID, "mpb_pack_text_device: bad arguments");
    if (n > 0x7fffffffll - 4096) return fail(MPB_E_INVALID, "batch of %lld reads exceeds 2^31; split it", (long long)n);
    if (row_stride <= 0 || row_stride % 16 != 0) return fail(MPB_E_INVALID, "row_stride must be a positive multiple of 16");
    if (row_stride > MPB_MAX_STRIDE) return fail(MPB_E_INVALID, "row_stride %lld exceeds %d (reads longer than %d bases are not supported)", (long long)row_stride, MPB_MAX_STRIDE, MPB_MAX_LEN);
    if (int orc = check_fastq_offset(fastq_offset)) return orc;
    if ((((uintptr_t)d_text | (uintptr_t)d_q_out) & 15) != 0) return fail(MPB_E_INVALID, "the text and the quality matrix must be 16-byte aligned");
    if ((((uintptr_t)d_rows | (uintptr_t)d_status) & 7) != 0 || ((uintptr_t)d_len_out & 3) != 0)
        return fail(MPB_E_INVALID, "the descriptors, the lengths and the status must be aligned to their element size");
    if (n == 0) return MPB_OK;
    if (!d_rows || !d_q_out || !d_len_out || !d_status || (text_bytes > 0 && !d_text)) return fail(MPB_E_INVALID, "NULL device buffer");
    { Span t(c, MPB_K_PACK_TEXT);
      mpb_launch_pack_text(d_text, text_bytes, d_rows, n, k0, fastq_offset, lower_n_is_base != 0, row_stride, d_q_out, d_len_out,
                           d_flags_out, d_status, c->stream); }
    HIPCHK(hipGetLastError());
    return MPB_OK;
}

int mpb_pack_text_device(mpb_ctx *c, const uint8_t *d_text, int64_t text_bytes, const mpb_text_row *d_rows, int64_t n,
                         int32_t fastq_offset, int32_t lower_n_is_base, int64_t row_stride, uint8_t *d_q_out,
                         int32_t *d_len_out, uint8_t *d_flags_out, int64_t *d_status)
{
    return pack_text_rows(c, d_text, text_bytes, d_rows, n, 0, fastq_offset, lower_n_is_base, row_stride, d_q_out, d_len_out,
                          d_flags_out, d_status);
}

int64_t text_piece_rows(int64_t n, int64_t stride)
{
    // (a smaller piece, for tests of the piece loop)
    int64_t piece_rows = env_int64("MPB_TEXT_PIECE_BYTES", 1, MPB_TEXT_PIECE_BYTES - 1, MPB_TEXT_PIECE_BYTES) / stride;
    if (piece_rows < 1) piece_rows = 1;
    if (piece_rows > n) piece_rows = n;
    return piece_rows;
}

int filter_text_pieces(StreamQueue &q, const uint8_t *d_text, int64_t text_bytes, const mpb_text_row *d_rows, int64_t n, int64_t stride,
                       int64_t piece_rows, int32_t fastq_offset, int32_t lower_n_is_base, const mpb_filter_params *params,
                       int32_t poisson, const TextStage &st, int64_t *n_pass_out, int64_t *n_overflow_out, int64_t *bad_record)
{
    mpb_ctx *c = q.c;
    const bool device_tail = poisson && !text_host_tail(params, poisson);
    char first_err[MPB_ERR_LEN] = "";                     // the message of the first filter call that failed
    int64_t *status = &c->pin->text_status[0];
    status[0] = status[1] = INT64_MAX;
    q.up(st.status, status, 2 * sizeof(int64_t));
    if (!q.ok()) return q.wait("hipMemcpyAsync (text upload)");          // (the caller's uploads among them: nothing is packed)
    // piece by piece: pack, look at the status, filter where the piece lies.  The status holds positions in row order (each piece
    // is packed with its first row's position as the base), and the pieces come in that order: the first piece that leaves it
    // dirty holds the first bad record, and nothing after it is packed or filtered.  mio_pack's error would have come before any
    // filter's: when a filter call fails, the pieces after it are still packed (not filtered) so that a bad quality there is seen.
    int rc = MPB_OK, wrc;
    int64_t n_pass = 0, n_overflow = 0;
    bool dirty = false;
    for (int64_t lo = 0; lo < n && !dirty; lo += piece_rows) {
        const int64_t m = n - lo < piece_rows ? n - lo : piece_rows;
        const int prc = pack_text_rows(c, d_text, text_bytes, d_rows + lo, m, lo, fastq_offset, lower_n_is_base, stride, st.q,
                                       st.len + lo, st.flags + lo, st.status);
        if (prc) return prc;
        q.down(status, st.status, 2 * sizeof(int64_t));
        if ((wrc = q.wait("hipMemcpyAsync (status)"))) return wrc;
        dirty = status[0] != INT64_MAX || status[1] != INT64_MAX;
        if (dirty || rc != MPB_OK) continue;
        mpb_filter_counts pc{};
        if (!poisson) rc = mpb_filter_device(c, st.q, m, stride, st.len + lo, 0, params, st.ee + lo, st.ns + lo, st.pass + lo, &pc);
        else if (device_tail) rc = mpb_filter_poisson_device(c, st.q, m, stride, st.len + lo, 0, params, st.ee + lo, st.ns + lo, st.pass + lo, nullptr, &pc);
        else rc = mpb_poisson_lambda_device(c, st.q, m, stride, st.len + lo, 0, st.ee + lo, st.ns + lo);     // (the host tail runs later)
        if (rc != MPB_OK) { strncpy(first_err, mpb_last_error(), sizeof(first_err) - 1); continue; }
        n_pass += pc.n_pass; n_overflow += pc.n_overflow;
    }
    if (dirty) {
        const int64_t first = status[0] < status[1] ? status[0] : status[1];
        if (bad_record) *bad_record = first;
        if (status[0] == first) return fail(MPB_E_RANGE, "Qualities must have positive values.");
        return fail(MPB_E_RANGE, "quality exceeds the encodable maximum 254");
    }
    if (rc) return fail(rc, "%s", first_err);
    *n_pass_out = n_pass; *n_overflow_out = n_overflow;
    return MPB_OK;
}

int text_results_queue(StreamQueue &q, const TextStage &st, int64_t n, bool host_tail, TextResults &r)
{
    if (host_tail && !r.len) {
        try { r.len_tmp.resize((size_t)n); } catch (const std::bad_alloc &) { return fail(MPB_E_NOMEM, "out of host memory"); }
    }
    int32_t *len_host = r.len_host();                             // (null when nobody wants the lengths)
    q.down(r.ee, st.ee, n * (int64_t)sizeof(double));
    q.down(r.ns, st.ns, n * (int64_t)sizeof(int32_t));
    if (!host_tail) q.down(r.pass, st.pass, n);
    if (len_host) q.down(len_host, st.len, n * (int64_t)sizeof(int32_t));
    if (r.flags) q.down(r.flags, st.flags, n);
    return MPB_OK;
}

int text_results_tail(int64_t n, const mpb_filter_params *params, bool host_tail, const TextResults &r, int64_t *n_pass)
{
    if (!host_tail) return MPB_OK;
    // the reference's scalar tail with the host's libm, in place: ee holds lambda (mpb_filter_poisson_host's arithmetic)
    const int rc = mpb_poisson_finish_host(r.ee, r.ns, r.len_host(), 0, n, params, r.ee, r.pass);
    if (rc || !n_pass) return rc;
    *n_pass = 0;
    for (int64_t i = 0; i < n; i++) *n_pass += r.pass[i];
    return MPB_OK;
}

int text_results_out(StreamQueue &q, const TextStage &st, int64_t n, const mpb_filter_params *params, int32_t poisson, TextResults &r,
                     int64_t *n_pass)
{
    const bool host_tail = text_host_tail(params, poisson);
    int rc;
    if ((rc = text_results_queue(q, st, n, host_tail, r))) return rc;
    if ((rc = q.wait("hipMemcpyAsync (results)"))) return rc;
    return text_results_tail(n, params, host_tail, r, n_pass);
}

int mpb_filter_text_host(mpb_ctx *c, const char *text, int64_t text_bytes, const int64_t *idx, int64_t n_records,
                         const int64_t *sel, int64_t n, int32_t fastq_offset, int32_t max_len, int32_t lower_n_is_base,
                         const mpb_filter_params *params, int32_t poisson, double *ee, int32_t *ns, uint8_t *pass,
                         int32_t *len_out, uint8_t *flags_out, mpb_filter_counts *counts, int64_t *bad_record)
{
    CTXCHK(c);
    if (bad_record) *bad_record = -1;
    int rc = check_params(params);
    if (rc) return rc;
    if (n < 0 || text_bytes < 0 || (text_bytes > 0 && !text)) return fail(MPB_E_INVALID, "mpb_filter_text_host: bad arguments");
    if (n > 0x7fffffffll - 4096) return fail(MPB_E_INVALID, "batch of %lld reads exceeds 2^31; split it", (long long)n);
    if (n > 0 && (!ee || !ns || !pass)) return fail(MPB_E_INVALID, "NULL host buffer");
    if ((rc = check_fastq_offset(fastq_offset))) return rc;
    // 1. the descriptors, validated on the host before anything is uploaded: first the longest packed length, then the rows
    int64_t longest = 0;
    if ((rc = mpb_text_rows(idx, n_records, sel, n, text_bytes, max_len, 0, nullptr, &longest, bad_record))) return rc;
    if (counts) { counts->n_reads = n; counts->n_pass = 0; counts->n_fail = 0; counts->n_overflow = 0; }
    if (n == 0) return MPB_OK;
    // 2. the ragged narrow pass' layout
    const int64_t stride = align_up(longest > 1 ? longest : 1, 128);
    // 3. (checked before anything is allocated)
    if ((rc = check_text_bytes(text_bytes))) return rc;
    std::vector<mpb_text_row> rows;
    try { rows.resize((size_t)n); } catch (const std::bad_alloc &) { return fail(MPB_E_NOMEM, "out of host memory for %lld row descriptors", (long long)n); }
    if ((rc = mpb_text_rows(idx, n_records, sel, n, text_bytes, max_len, stride, rows.data(), nullptr, bad_record))) return rc;
    const int64_t piece_rows = text_piece_rows(n, stride);
    TextStage st{};
    if ((rc = carve(c, c->text_stage, [&](Carver &k) { st.layout(k, text_bytes, n, piece_rows, stride); }))) return rc;
    // 4. the uploads (the queue leaves before `rows` and `res`, which it copies from and into)
    TextResults res{ee, ns, pass, len_out, flags_out, {}};
    StreamQueue q(c);
    q.up(st.text, text, text_bytes);
    q.up(st.rows, rows.data(), n * (int64_t)sizeof(mpb_text_row));
    // 5. the piece loop (above)
    int64_t n_pass = 0, n_overflow = 0;
    if ((rc = filter_text_pieces(q, st.text, text_bytes, st.rows, n, stride, piece_rows, fastq_offset, lower_n_is_base, params, poisson,
                                 st, &n_pass, &n_overflow, bad_record))) return rc;
    if ((rc = text_results_out(q, st, n, params, poisson, res, &n_pass))) return rc;
    if (counts) { counts->n_pass = n_pass; counts->n_fail = n - n_pass; counts->n_overflow = n_overflow; }
    return MPB_OK;
}
