// mpb_text.cpp -- FASTQ text as it lies in the file, behind the C ABI of libmoira_pb.so (include/moira_pb.h): the device pack
// from a text buffer and its validated row descriptors (k_pack_text), and the host entry that uploads a chunk's text once,
// packs it on the device and filters it there.  The descriptors come from mpb_text_rows (mpb_hostonly.cpp).  The piece loop
// (filter_text_pieces) takes a text and descriptors that are on the device already: mpb_contig.cpp runs it over contig slots.
// (Every mpb_* function defined here has C linkage: include/moira_pb.h declares it inside extern "C".)

#include "mpb_ctx.h"

#include <cstdlib>
#include <cstring>
#include <vector>

#define MPB_TEXT_MAX_BYTES (1ll << 30)       // the text of one mpb_filter_text_host call
#define MPB_TEXT_PIECE_BYTES (256ll << 20)   // ... and the piece of the matrix that is packed and filtered at a time

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
    if (fastq_offset < 0 || fastq_offset > 255)
        return fail(MPB_E_INVALID, "fastq_offset %d: the device pack takes offsets 0..255 (beyond them no character is a quality)", fastq_offset);
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
    int64_t lim = MPB_TEXT_PIECE_BYTES;
    if (const char *e = getenv("MPB_TEXT_PIECE_BYTES")) {          // a smaller piece, for tests of the piece loop
        const long long v = atoll(e);
        if (v > 0 && v < lim) lim = v;
    }
    int64_t piece_rows = lim / stride;
    if (piece_rows < 1) piece_rows = 1;
    if (piece_rows > n) piece_rows = n;
    return piece_rows;
}

int filter_text_pieces(mpb_ctx *c, const uint8_t *d_text, int64_t text_bytes, const mpb_text_row *d_rows, int64_t n, int64_t stride,
                       int64_t piece_rows, int32_t fastq_offset, int32_t lower_n_is_base, const mpb_filter_params *params,
                       int32_t poisson, const TextStage &st, int64_t *n_pass_out, int64_t *n_overflow_out, int64_t *bad_record)
{
    const bool device_tail = poisson && params && (params->flags & MPB_FLAG_POISSON_DEVICE_TAIL);
    hipStream_t s = c->stream;
    char first_err[MPB_ERR_LEN] = "";                     // the message of the first filter call that failed
    int64_t *status = &c->pin->text_status[0];
    status[0] = status[1] = INT64_MAX;
    // (everything below is queued on one stream; the host blocks it reads from -- the pinned words -- outlive the synchronisation
    // that every path out of here passes)
    const hipError_t e_up = hipMemcpyAsync(st.status, status, 2 * sizeof(int64_t), hipMemcpyHostToDevice, s);
    if (e_up != hipSuccess) { (void)hipStreamSynchronize(s); return hip_fail("hipMemcpyAsync (text upload)", e_up); }
    // piece by piece: pack, look at the status, filter where the piece lies.  The status holds positions in row order (each piece
    // is packed with its first row's position as the base), and the pieces come in that order: the first piece that leaves it
    // dirty holds the first bad record, and nothing after it is packed or filtered.  mio_pack's error would have come before any
    // filter's: when a filter call fails, the pieces after it are still packed (not filtered) so that a bad quality there is seen.
    int rc = MPB_OK;
    int64_t n_pass = 0, n_overflow = 0;
    bool dirty = false;
    for (int64_t lo = 0; lo < n && !dirty; lo += piece_rows) {
        const int64_t m = n - lo < piece_rows ? n - lo : piece_rows;
        const int prc = pack_text_rows(c, d_text, text_bytes, d_rows + lo, m, lo, fastq_offset, lower_n_is_base, stride, st.q,
                                       st.len + lo, st.flags + lo, st.status);
        if (prc) { (void)hipStreamSynchronize(s); return prc; }
        const hipError_t e_st = hipMemcpyAsync(status, st.status, 2 * sizeof(int64_t), hipMemcpyDeviceToHost, s);
        const hipError_t e_sync = hipStreamSynchronize(s);
        HIPCHK_KEPT("hipMemcpyAsync (status)", e_st);
        HIPCHK_KEPT("hipStreamSynchronize", e_sync);
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
    if (rc) { (void)hipStreamSynchronize(s); return fail(rc, "%s", first_err); }
    *n_pass_out = n_pass; *n_overflow_out = n_overflow;
    return MPB_OK;
}

int text_results_out(mpb_ctx *c, const TextStage &st, int64_t n, const mpb_filter_params *params, int32_t poisson, double *ee,
                     int32_t *ns, uint8_t *pass, int32_t *len_out, uint8_t *flags_out, int64_t *n_pass_io)
{
    const bool device_tail = poisson && params && (params->flags & MPB_FLAG_POISSON_DEVICE_TAIL);
    hipStream_t s = c->stream;
    int rc;
    int64_t n_pass = *n_pass_io;
    // the results, whole
    hipError_t e_out = hipMemcpyAsync(ee, st.ee, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s);
    if (e_out == hipSuccess) e_out = hipMemcpyAsync(ns, st.ns, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, s);
    if (e_out == hipSuccess && !(poisson && !device_tail)) e_out = hipMemcpyAsync(pass, st.pass, (size_t)n, hipMemcpyDeviceToHost, s);
    std::vector<int32_t> len_tmp;
    int32_t *len_host = len_out;
    if (poisson && !device_tail && !len_host) {
        try { len_tmp.resize((size_t)n); } catch (const std::bad_alloc &) { (void)hipStreamSynchronize(s); return fail(MPB_E_NOMEM, "out of host memory"); }
        len_host = len_tmp.data();
    }
    if (e_out == hipSuccess && len_host) e_out = hipMemcpyAsync(len_host, st.len, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, s);
    if (e_out == hipSuccess && flags_out) e_out = hipMemcpyAsync(flags_out, st.flags, (size_t)n, hipMemcpyDeviceToHost, s);
    const hipError_t e_sync = hipStreamSynchronize(s);
    HIPCHK_KEPT("hipMemcpyAsync (results)", e_out);
    HIPCHK_KEPT("hipStreamSynchronize", e_sync);
    if (poisson && !device_tail) {
        // the reference's scalar tail with the host's libm, in place: ee holds lambda (mpb_filter_poisson_host's arithmetic)
        if ((rc = mpb_poisson_finish_host(ee, ns, len_host, 0, n, params, ee, pass))) return rc;
        n_pass = 0;
        for (int64_t i = 0; i < n; i++) n_pass += pass[i];
    }
    *n_pass_io = n_pass;
    return MPB_OK;
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
    if (fastq_offset < 0 || fastq_offset > 255)
        return fail(MPB_E_INVALID, "fastq_offset %d: the device pack takes offsets 0..255 (beyond them no character is a quality)", fastq_offset);
    // 1. the descriptors, validated on the host before anything is uploaded: first the longest packed length, then the rows
    int64_t longest = 0;
    if ((rc = mpb_text_rows(idx, n_records, sel, n, text_bytes, max_len, 0, nullptr, &longest, bad_record))) return rc;
    if (counts) { counts->n_reads = n; counts->n_pass = 0; counts->n_fail = 0; counts->n_overflow = 0; }
    if (n == 0) return MPB_OK;
    // 2. the ragged narrow pass' layout
    const int64_t stride = align_up(longest > 1 ? longest : 1, 128);
    // 3. (checked before anything is allocated)
    if (text_bytes > MPB_TEXT_MAX_BYTES)
        return fail(MPB_E_INVALID, "text of %lld bytes: one call takes at most %lld bytes (1 GiB) of text; split the chunk",
                    (long long)text_bytes, (long long)MPB_TEXT_MAX_BYTES);
    std::vector<mpb_text_row> rows;
    try { rows.resize((size_t)n); } catch (const std::bad_alloc &) { return fail(MPB_E_NOMEM, "out of host memory for %lld row descriptors", (long long)n); }
    if ((rc = mpb_text_rows(idx, n_records, sel, n, text_bytes, max_len, stride, rows.data(), nullptr, bad_record))) return rc;
    const int64_t piece_rows = text_piece_rows(n, stride);
    TextStage st{};
    if ((rc = carve(c, c->text_stage, [&](Carver &k) { st.layout(k, text_bytes, n, piece_rows, stride); }))) return rc;
    hipStream_t s = c->stream;
    // (everything below is queued on one stream; the host blocks it reads from -- the caller's text, `rows` -- outlive the
    // synchronisation that every path out of here passes)
    hipError_t e_up = hipSuccess;
    if (text_bytes > 0) e_up = hipMemcpyAsync(st.text, text, (size_t)text_bytes, hipMemcpyHostToDevice, s);
    if (e_up == hipSuccess) e_up = hipMemcpyAsync(st.rows, rows.data(), (size_t)n * sizeof(mpb_text_row), hipMemcpyHostToDevice, s);
    if (e_up != hipSuccess) { (void)hipStreamSynchronize(s); return hip_fail("hipMemcpyAsync (text upload)", e_up); }
    // 5. the piece loop (above)
    int64_t n_pass = 0, n_overflow = 0;
    if ((rc = filter_text_pieces(c, st.text, text_bytes, st.rows, n, stride, piece_rows, fastq_offset, lower_n_is_base, params, poisson,
                                 st, &n_pass, &n_overflow, bad_record))) return rc;
    if ((rc = text_results_out(c, st, n, params, poisson, ee, ns, pass, len_out, flags_out, &n_pass))) return rc;
    if (counts) { counts->n_pass = n_pass; counts->n_fail = n - n_pass; counts->n_overflow = n_overflow; }
    return MPB_OK;
}
