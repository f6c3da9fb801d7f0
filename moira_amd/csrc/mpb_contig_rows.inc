// mpb_contig_rows.inc -- what ONE THREAD of k_contig_rows does (mpb_contig_kernels.hip): the row descriptor k_pack_text walks for
// pair i, from done[i] and row i of the index k_contig wrote (mpb_contigs_filter_text_host).  No intrinsic lives here.  The
// includer defines CR_FN (the function attributes), cr_done(done, i) and cr_idx(out_idx, k) (one element of either array);
// tests/helpers/contig_rows_check.cpp compiles the file on the host with accessors that check i and k against the arrays.
//
// The index is written by the device and is still not trusted: a row is handed on only when its length is mpb_text_rows' (the
// quality length, cut to max_len when max_len > 0), lies in 0..min(65535, stride), and both lines lie inside the pair's OWN slot
// [i * rec_cap, (i + 1) * rec_cap).  Anything else is {0, 0, -1}, which k_pack_text turns into a zero row of length -1.  A pair
// the device handed back (done == 0) is an empty read: its index row is never looked at and its results are never reported.

CR_FN mpb_text_row cr_row(const int64_t *out_idx, const uint8_t *done, int64_t i, int64_t rec_cap, int32_t max_len, int64_t stride)
{
    mpb_text_row r;
    r.seq_off = 0; r.qual_off = 0; r.len = 0; r.pad = 0;
    if (!cr_done(done, i)) return r;
    const int64_t so = cr_idx(out_idx, i * MPB_IDX_COLS + MPB_IDX_SEQ_OFF), sl = cr_idx(out_idx, i * MPB_IDX_COLS + 3);
    const int64_t qo = cr_idx(out_idx, i * MPB_IDX_COLS + MPB_IDX_QUAL_OFF), ql = cr_idx(out_idx, i * MPB_IDX_COLS + MPB_IDX_QUAL_LEN);
    int64_t len = ql;
    if (max_len > 0 && len > max_len) len = max_len;                 // mio_pack's rule
    const int64_t lo = i * rec_cap;                                  // (i < n and n * rec_cap is the slot buffer's size: no overflow)
    const int64_t most = stride < 65535 ? stride : 65535;
    // (every difference below is taken only after the comparison that keeps it inside 0..INT64_MAX)
    const bool ok = sl == ql && len >= 0 && len <= most && len <= rec_cap &&
                    so >= lo && so - lo <= rec_cap - len && qo >= lo && qo - lo <= rec_cap - len;
    if (!ok) { r.len = -1; return r; }
    r.seq_off = so; r.qual_off = qo; r.len = (int32_t)len;
    return r;
}
