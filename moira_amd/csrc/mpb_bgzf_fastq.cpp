// mpb_bgzf_fastq.cpp -- BGZF FASTQ filtered where it inflates, behind the C ABI of libmoira_pb.so (include/moira_pb.h): the entry
// that takes compressed members and returns the filter's results (mpb_filter_bgzf_fastq_host: k_bgzf_inflate writes the text
// straight into the device index's stage, k_bgzf_crc32 vouches for it there, and mpb_index.cpp's kernels and mpb_text.cpp's piece
// loop go on from it), and the CRC-32 of ranges of a text (mpb_crc32_ranges_host: the CRC kernel's own entry).  Both launch
// k_bgzf_crc32 (mpb_crc_kernels.hip) inside the timing span of MPB_K_BGZF_INFLATE: the kernel has no id of its own.
// (Every mpb_* function defined here has C linkage: include/moira_pb.h declares it inside extern "C".)

#include "mpb_ctx.h"

#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

namespace {

// text | ranges | CRC words and markers: the CRC entry's own call
struct CrcStage {
    uint8_t *text; mpb_crc_range *ranges; uint32_t *crcw;
    void layout(Carver &k, int64_t text_bytes, int64_t n)
    {
        k.take(text, align_up(text_bytes > 0 ? text_bytes : 1, 16));
        k.take(ranges, n);
        k.take(crcw, 2 * n);
    }
};

// compressed bytes | rows | status rows | ranges | CRC words and markers (the text lies in the index's stage)
struct FusedStage {
    uint8_t *in; mpb_bgzf_member_row *rows; uint32_t *mstat; mpb_crc_range *ranges; uint32_t *crcw;
    void layout(Carver &k, int64_t in_bytes, int64_t members)
    {
        const int64_t m = members > 0 ? members : 1;
        k.take(in, align_up(in_bytes > 0 ? in_bytes : 1, 16));
        k.take(rows, m);
        k.take(mstat, m * MPB_INFLATE_MSTAT);
        k.take(ranges, m);
        k.take(crcw, 2 * m);
    }
};

}  // namespace

int mpb_crc32_ranges_host(mpb_ctx *c, const uint8_t *text, int64_t text_bytes, const int64_t *offs, const int32_t *lens, int64_t n,
                          uint32_t *crc_out)
{
    // (the arguments first: what is wrong with them is said with or without a device)
    if (n < 0 || text_bytes < 0 || (text_bytes > 0 && !text) || (n > 0 && (!offs || !lens || !crc_out)))
        return fail(MPB_E_INVALID, "mpb_crc32_ranges_host: bad arguments");
    if (text_bytes > k_text_max_bytes)
        return fail(MPB_E_INVALID, "mpb_crc32_ranges_host: text of %lld bytes: one call takes at most %lld bytes (1 GiB)",
                    (long long)text_bytes, (long long)k_text_max_bytes);
    for (int64_t k = 0; k < n; k++)
        if (offs[k] < 0 || lens[k] < 0 || lens[k] > MPB_CRC_RANGE_MAX || offs[k] > text_bytes - (int64_t)lens[k])
            return fail(MPB_E_INVALID, "mpb_crc32_ranges_host: range %lld (offset %lld, %d bytes) does not lie inside the %lld bytes of text, or is longer than %d",
                        (long long)k, (long long)offs[k], (int)lens[k], (long long)text_bytes, MPB_CRC_RANGE_MAX);
    CTXCHK(c);
    if (n == 0) return MPB_OK;
    std::vector<mpb_crc_range> ranges;
    std::vector<uint32_t> crcw;
    try { ranges.resize((size_t)n); crcw.resize((size_t)n * 2); }
    catch (const std::bad_alloc &) { return fail(MPB_E_NOMEM, "out of host memory for %lld ranges", (long long)n); }
    for (int64_t k = 0; k < n; k++) ranges[(size_t)k] = mpb_crc_range{offs[k], lens[k], 0};
    CrcStage st{};
    int rc;
    if ((rc = carve(c, c->inflate_stage, [&](Carver &k) { st.layout(k, text_bytes, n); }))) return rc;
    hipStream_t s = c->stream;
    // (everything below is queued on one stream; the host blocks it reads from outlive the synchronisation)
    hipError_t e = text_bytes > 0 ? hipMemcpyAsync(st.text, text, (size_t)text_bytes, hipMemcpyHostToDevice, s) : hipSuccess;
    if (e == hipSuccess) e = hipMemcpyAsync(st.ranges, ranges.data(), (size_t)n * sizeof(mpb_crc_range), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) {
        { Span t(c, MPB_K_BGZF_INFLATE); mpb_launch_bgzf_crc32(st.text, text_bytes, st.ranges, n, st.crcw, st.crcw + n, s); }
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(crcw.data(), st.crcw, (size_t)n * 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, s);
    const hipError_t e_sync = hipStreamSynchronize(s);
    HIPCHK_KEPT("k_bgzf_crc32 / hipMemcpyAsync (crc ranges)", e);
    HIPCHK_KEPT("hipStreamSynchronize", e_sync);
    for (int64_t k = 0; k < n; k++)
        if (crcw[(size_t)(n + k)] != 0)
            return fail(MPB_E_INVALID, "mpb_crc32_ranges_host: the kernel refused range %lld (never expected)", (long long)k);
    memcpy(crc_out, crcw.data(), (size_t)n * sizeof(uint32_t));
    return MPB_OK;
}

int mpb_filter_bgzf_fastq_host(mpb_ctx *c, const char *carry, int64_t carry_len, const uint8_t *in, int64_t in_len, const int64_t *offs,
                               const int32_t *sizes, const int64_t *out_offs, int64_t n_members, int32_t final, int64_t max_records,
                               int32_t max_len, uint8_t *text_out, int64_t text_cap, uint8_t *done, uint8_t *member_why,
                               int64_t *first_back, mpb_bgzf_inflate_stats *stats, int64_t *idx_out, int64_t idx_cap_rows, int64_t *n,
                               int64_t *consumed, int32_t *bad_kind, int32_t *why, int32_t fastq_offset, int32_t lower_n_is_base,
                               const mpb_filter_params *params, int32_t poisson, double *ee, int32_t *ns, uint8_t *pass,
                               int32_t *len_out, uint8_t *flags_out, mpb_filter_counts *counts, int64_t *bad_record)
{
    // 1. the arguments: what is wrong with them is said with or without a device
    if (bad_record) *bad_record = -1;
    int rc = check_params(params);
    if (rc) return rc;
    if (carry_len < 0 || (carry_len > 0 && !carry) || in_len < 0 || n_members < 0 || !out_offs ||
        (n_members > 0 && (!in || !offs || !sizes || !done)) || max_records < 0 || max_len < 0 || text_cap < 0 || !first_back ||
        idx_cap_rows < 1 || !idx_out || !n || !consumed || !bad_kind || !why || !ee || !ns || !pass)
        return fail(MPB_E_INVALID, "mpb_filter_bgzf_fastq_host: bad arguments");
    if (out_offs[0] != 0 || out_offs[n_members] < 0)
        return fail(MPB_E_INVALID, "mpb_filter_bgzf_fastq_host: out_offs must start at 0 (the members' text follows the carry)");
    if (carry_len > k_text_max_bytes || out_offs[n_members] > k_text_max_bytes - carry_len)
        return fail(MPB_E_INVALID, "mpb_filter_bgzf_fastq_host: text of %lld + %lld bytes: one call takes at most %lld bytes (1 GiB) of text; "
                    "split the batch", (long long)carry_len, (long long)out_offs[n_members], (long long)k_text_max_bytes);
    const int64_t T = carry_len + out_offs[n_members];
    if (text_out && text_cap < T)
        return fail(MPB_E_INVALID, "mpb_filter_bgzf_fastq_host: text_cap %lld is below the %lld bytes of text", (long long)text_cap, (long long)T);
    if (fastq_offset < 0 || fastq_offset > 255)
        return fail(MPB_E_INVALID, "mpb_filter_bgzf_fastq_host: fastq_offset %d: the device pack takes offsets 0..255 (beyond them no "
                    "character is a quality)", fastq_offset);
    // 2. the rows: the only place a member's offsets are trusted from
    std::vector<mpb_bgzf_member_row> rows;
    std::vector<mpb_crc_range> ranges;
    std::vector<uint32_t> crc, mstat, crcw;
    std::vector<uint8_t> reason;
    try {
        rows.resize((size_t)n_members); ranges.resize((size_t)n_members); crc.resize((size_t)n_members); reason.resize((size_t)n_members);
        mstat.resize((size_t)n_members * MPB_INFLATE_MSTAT); crcw.resize((size_t)n_members * 2);
    } catch (const std::bad_alloc &) { return fail(MPB_E_NOMEM, "out of host memory for %lld members", (long long)n_members); }
    if ((rc = mpb_bgzf_member_rows(in, in_len, offs, sizes, out_offs, n_members, rows.data(), crc.data(), reason.data()))) return rc;
    CTXCHK(c);
    *first_back = -1; *n = 0; *consumed = 0; *bad_kind = 0; *why = MPB_FQ_WHY_TAKEN;
    if (counts) memset(counts, 0, sizeof(*counts));
    if (stats) { memset(stats, 0, sizeof(*stats)); stats->members = n_members; stats->handed_back = n_members; }
    if (n_members > 0) memset(done, 0, (size_t)n_members);
    int64_t in_lo = 0, in_hi = 0;                            // the one range of `in` that holds every vouched-for stream
    bool any = false;
    for (int64_t k = 0; k < n_members; k++) {
        const mpb_bgzf_member_row &r = rows[(size_t)k];
        if (r.out_len < 0) continue;
        in_lo = any ? std::min(in_lo, r.stream_off) : r.stream_off;
        in_hi = any ? std::max(in_hi, r.stream_off + r.stream_len) : r.stream_off + r.stream_len;
        any = true;
    }
    for (int64_t k = 0; k < n_members; k++) {               // ... relative to that range, and to the text behind the carry
        mpb_bgzf_member_row &r = rows[(size_t)k];
        ranges[(size_t)k] = mpb_crc_range{0, 0, 0};
        if (r.out_len < 0) continue;
        r.stream_off -= in_lo; r.out_off += carry_len;
        ranges[(size_t)k] = mpb_crc_range{r.out_off, r.out_len, 0};
    }
    // 3. the stages: the text is the index's; compressed bytes, rows, status rows and CRC words are the inflater's
    const int64_t n_tiles = (T + MPB_FQ_TILE - 1) / MPB_FQ_TILE, in_bytes = in_hi - in_lo;
    Indexed ind;
    FusedStage fs{};
    if ((rc = carve(c, c->fastq_stage, [&](Carver &k) { ind.st.layout(k, T, n_tiles); }))) return rc;
    if ((rc = carve(c, c->inflate_stage, [&](Carver &k) { fs.layout(k, in_bytes, n_members); }))) return rc;
    hipStream_t s = c->stream;
    uint8_t *d_text = ind.st.text;
    // 4. - 6. upload, inflate, CRC; the index's first two kernels behind them, so that one synchronisation serves members and head
    // words (everything is queued on one stream; the host blocks it reads from outlive the synchronisation)
    hipError_t e = carry_len > 0 ? hipMemcpyAsync(d_text, carry, (size_t)carry_len, hipMemcpyHostToDevice, s) : hipSuccess;
    if (e == hipSuccess && in_bytes > 0) e = hipMemcpyAsync(fs.in, in + in_lo, (size_t)in_bytes, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && n_members > 0) e = hipMemcpyAsync(fs.rows, rows.data(), (size_t)n_members * sizeof(mpb_bgzf_member_row), hipMemcpyHostToDevice, s);
    if (e == hipSuccess && n_members > 0) e = hipMemcpyAsync(fs.ranges, ranges.data(), (size_t)n_members * sizeof(mpb_crc_range), hipMemcpyHostToDevice, s);
    if (e == hipSuccess && n_members > 0) {
        { Span t(c, MPB_K_BGZF_INFLATE);
          mpb_launch_bgzf_inflate(fs.in, in_bytes, fs.rows, n_members, d_text, T, fs.mstat, s);
          // (over every vouched-for member, taken or not: the range of one that was not taken holds whatever the block held, and
          // its CRC word is not looked at)
          mpb_launch_bgzf_crc32(d_text, T, fs.ranges, n_members, fs.crcw, fs.crcw + n_members, s); }
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(mstat.data(), fs.mstat, (size_t)n_members * MPB_INFLATE_MSTAT * sizeof(uint32_t), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(crcw.data(), fs.crcw, (size_t)n_members * 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, s);
    }
    if (e == hipSuccess) e = fastq_index_queue_head(c, ind, T, final);
    const hipError_t e_sync = hipStreamSynchronize(s);
    HIPCHK_KEPT("k_bgzf_inflate / k_bgzf_crc32 / k_fq_lines / k_fq_scan", e);
    HIPCHK_KEPT("hipStreamSynchronize", e_sync);
    // 7. the decision: all or nothing
    int64_t taken = 0;
    mpb_bgzf_inflate_stats acc;
    memset(&acc, 0, sizeof(acc));
    for (int64_t k = 0; k < n_members; k++) {
        if (rows[(size_t)k].out_len < 0) { if (*first_back < 0) *first_back = k; continue; }       // (reason: MPB_BGZF_WHY_HEADER)
        const uint32_t *ms = &mstat[(size_t)k * MPB_INFLATE_MSTAT];
        const uint32_t w = ms[0];
        reason[(size_t)k] = (uint8_t)(w <= MPB_BGZF_WHY_TRAILING_BYTES ? w : MPB_BGZF_WHY_HEADER);
        if (w == MPB_BGZF_WHY_OK && (crcw[(size_t)(n_members + k)] != 0 || crcw[(size_t)k] != crc[(size_t)k])) reason[(size_t)k] = MPB_BGZF_WHY_CRC;
        if (reason[(size_t)k] != MPB_BGZF_WHY_OK) { if (*first_back < 0) *first_back = k; continue; }
        done[k] = 1;
        taken++;
        acc.stored_blocks += ms[1]; acc.fixed_blocks += ms[2]; acc.dynamic_blocks += ms[3];
        acc.literals += ms[4]; acc.matches += ms[5]; acc.matched_bytes += ms[6];
        acc.longest_code = std::max(acc.longest_code, (int64_t)ms[7]);
    }
    if (member_why && n_members > 0) memcpy(member_why, reason.data(), (size_t)n_members);
    if (stats) { *stats = acc; stats->members = n_members; stats->taken = taken; stats->handed_back = n_members - taken; }
    if (*first_back >= 0) return MPB_OK;                     // (what k_fq_lines / k_fq_scan made of the text is dropped with it)
    // 8. index, pack, filter over the text where it lies: mpb_filter_fastq_host's steps
    if ((rc = fastq_index_finish(c, T, max_records, max_len, idx_cap_rows, n, ind, why))) return rc;
    *n = 0;
    if (*why) return MPB_OK;
    if (ind.n > 0x7fffffffll - 4096) return fail(MPB_E_INVALID, "batch of %lld reads exceeds 2^31; split it", (long long)ind.n);
    if (ind.longest > MPB_MAX_LEN)
        return fail(MPB_E_INVALID, "reads longer than 65535 bases are not supported; length (%lld)", (long long)ind.longest);
    int64_t n_pass = 0, n_overflow = 0;
    TextStage st{};
    if (ind.n > 0) {
        const int64_t stride = align_up(ind.longest > 1 ? ind.longest : 1, 128);
        const int64_t piece_rows = text_piece_rows(ind.n, stride);
        if ((rc = carve(c, c->text_stage, [&](Carver &k) { st.layout_results(k, ind.n, piece_rows, stride); }))) return rc;
        if ((rc = filter_text_pieces(c, d_text, T, ind.ix.desc, ind.n, stride, piece_rows, fastq_offset, lower_n_is_base, params, poisson, st,
                                     &n_pass, &n_overflow, bad_record))) return rc;
    }
    uint32_t *consumed32 = &c->pin->fq_head[0];
    uint8_t *kind8 = (uint8_t *)&c->pin->fq_head[1];
    *consumed32 = 0; *kind8 = 0;
    e = queue_index_out(c, ind, idx_out, consumed32, kind8);
    if (e == hipSuccess && text_out && T > 0) e = hipMemcpyAsync(text_out, d_text, (size_t)T, hipMemcpyDeviceToHost, s);
    if (e != hipSuccess) { (void)hipStreamSynchronize(s); return hip_fail("hipMemcpyAsync (index, text)", e); }
    if (ind.n > 0) {
        if ((rc = text_results_out(c, st, ind.n, params, poisson, ee, ns, pass, len_out, flags_out, &n_pass))) return rc;
    } else {
        HIPCHK(hipStreamSynchronize(s));
    }
    *n = ind.n; *consumed = (int64_t)*consumed32; *bad_kind = (int32_t)*kind8;
    if (counts) { counts->n_reads = ind.n; counts->n_pass = n_pass; counts->n_fail = ind.n - n_pass; counts->n_overflow = n_overflow; }
    return MPB_OK;
}
