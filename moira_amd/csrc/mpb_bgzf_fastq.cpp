// mpb_bgzf_fastq.cpp -- BGZF FASTQ filtered where it inflates, behind the C ABI of libmoira_pb.so (include/moira_pb.h): the entry
// that takes compressed members and returns the filter's results (mpb_filter_bgzf_fastq_host: k_bgzf_inflate writes the text
// straight into the device index's stage, k_bgzf_crc32 vouches for it there, and mpb_index.cpp's kernels and mpb_text.cpp's piece
// loop go on from it), and the CRC-32 of ranges of a text (mpb_crc32_ranges_host: the CRC kernel's own entry).  Both launch
// k_bgzf_crc32 (mpb_crc_kernels.hip) inside the timing span of MPB_K_BGZF_INFLATE: the kernel has no id of its own.  Each entry
// queues on one StreamQueue (mpb_queue.h); the members' verdict is mpb_hostonly.cpp's, the filter tail mpb_index.cpp's.
// (Every mpb_* function defined here has C linkage: include/moira_pb.h declares it inside extern "C".)

#include "mpb_ctx.h"

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
    StreamQueue q(c);
    q.up(st.text, text, text_bytes);
    q.up(st.ranges, ranges.data(), n * (int64_t)sizeof(mpb_crc_range));
    q.run(MPB_K_BGZF_INFLATE, [&] { mpb_launch_bgzf_crc32(st.text, text_bytes, st.ranges, n, st.crcw, st.crcw + n, s); });
    q.down(crcw.data(), st.crcw, n * 2 * (int64_t)sizeof(uint32_t));
    if ((rc = q.wait("k_bgzf_crc32 / hipMemcpyAsync (crc ranges)"))) return rc;
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
    if ((rc = check_fastq_offset(fastq_offset, "mpb_filter_bgzf_fastq_host"))) return rc;
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
    resident_drop(c);
    *first_back = -1; *n = 0; *consumed = 0; *bad_kind = 0; *why = MPB_FQ_WHY_TAKEN;
    if (counts) memset(counts, 0, sizeof(*counts));
    if (stats) { memset(stats, 0, sizeof(*stats)); stats->members = n_members; stats->handed_back = n_members; }
    if (n_members > 0) memset(done, 0, (size_t)n_members);
    int64_t in_lo = 0, in_hi = 0;                            // the one range of `in` that holds every vouched-for stream
    bgzf_stream_range(rows.data(), n_members, false, &in_lo, &in_hi);
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
    // 4. - 6. upload, inflate, CRC; the index's first two kernels behind them, so that one wait serves members and head words
    // (the queue leaves before the vectors and `res`, which it copies from and into)
    TextResults res{ee, ns, pass, len_out, flags_out, {}};
    StreamQueue q(c);
    q.up(d_text, carry, carry_len);
    q.up(fs.in, in + in_lo, in_bytes);
    q.up(fs.rows, rows.data(), n_members * (int64_t)sizeof(mpb_bgzf_member_row));
    q.up(fs.ranges, ranges.data(), n_members * (int64_t)sizeof(mpb_crc_range));
    if (n_members > 0) {
        q.run(MPB_K_BGZF_INFLATE, [&] {
            mpb_launch_bgzf_inflate(fs.in, in_bytes, fs.rows, n_members, d_text, T, fs.mstat, s);
            // (over every vouched-for member, taken or not: the range of one that was not taken holds whatever the block held, and
            // its CRC word is not looked at)
            mpb_launch_bgzf_crc32(d_text, T, fs.ranges, n_members, fs.crcw, fs.crcw + n_members, s); });
        q.down(mstat.data(), fs.mstat, n_members * MPB_INFLATE_MSTAT * (int64_t)sizeof(uint32_t));
        q.down(crcw.data(), fs.crcw, n_members * 2 * (int64_t)sizeof(uint32_t));
    }
    fastq_index_queue_head(q, ind, T, final);
    if ((rc = q.wait("k_bgzf_inflate / k_bgzf_crc32 / k_fq_lines / k_fq_scan"))) return rc;
    // 7. the decision: all or nothing
    mpb_bgzf_inflate_stats acc;
    memset(&acc, 0, sizeof(acc));
    for (int64_t k = 0; k < n_members; k++) {
        if (rows[(size_t)k].out_len < 0) { if (*first_back < 0) *first_back = k; continue; }       // (reason: MPB_BGZF_WHY_HEADER)
        const uint32_t *ms = &mstat[(size_t)k * MPB_INFLATE_MSTAT];
        reason[(size_t)k] = bgzf_member_reason(ms[0]);
        if (ms[0] == MPB_BGZF_WHY_OK && (crcw[(size_t)(n_members + k)] != 0 || crcw[(size_t)k] != crc[(size_t)k])) reason[(size_t)k] = MPB_BGZF_WHY_CRC;
        if (reason[(size_t)k] != MPB_BGZF_WHY_OK) { if (*first_back < 0) *first_back = k; continue; }
        done[k] = 1;
        bgzf_stats_add(&acc, ms);
    }
    if (member_why && n_members > 0) memcpy(member_why, reason.data(), (size_t)n_members);
    if (stats) { *stats = acc; stats->members = n_members; stats->handed_back = n_members - acc.taken; }
    if (*first_back >= 0) return MPB_OK;                     // (what k_fq_lines / k_fq_scan made of the text is dropped with it)
    // 8. index, pack, filter over the text where it lies: mpb_filter_fastq_host's steps
    if ((rc = fastq_index_finish(q, T, max_records, max_len, idx_cap_rows, n, ind, why))) return rc;
    *n = 0;
    if (*why) return MPB_OK;
    return filter_indexed(q, ind, T, text_out, idx_out, n, consumed, bad_kind,
                          FastqFilterAsk{fastq_offset, lower_n_is_base, params, poisson, counts, bad_record}, res);
}
