// mpb_format.cpp -- the writer's formatter on the device, behind the C ABI of libmoira_pb.so (include/moira_pb.h): the entry that
// turns selected records of a text and its record index into fasta, qual or fastq text (mpb_format_text_host), from an upload
// or from what the last filter call left on the device (the resident form), and hands back the text or -- compressed where it
// lies by mpb_bgzf.cpp's piece -- its BGZF members.  The kernels are mpb_format_kernels.hip (k_fmt_count, k_fmt_scan, k_fmt_write,
// inside MPB_K_PACK_TEXT's span: they have no id of their own); what a lane does, and the row checks the host makes first, are
// mpb_format_lane.inc.  mio_format (csrc/fastio.cpp) defines the output.  The entry queues on one StreamQueue (mpb_queue.h).
// (Every mpb_* function defined here has C linkage: include/moira_pb.h declares it inside extern "C".)

#include "mpb_ctx.h"

#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

// the lane code on the host: fm_row is the validation of an uploaded index (the words of a text are never asked for here)
#define FM_FN static inline
#define FM_LD_I64(p, k) ((p)[k])
#define FM_LD_I32(p, k) ((p)[k])
#define FM_LD16(text, off) fm_hload16((text) + (off))
struct fm_w16;
static inline fm_w16 fm_hload16(const uint8_t *p);
#include "mpb_format_lane.inc"
static inline fm_w16 fm_hload16(const uint8_t *p)
{
    fm_w16 o;
    memcpy(o.w, p, 16);
    return o;
}

#define MPB_FORMAT_PIECE_BYTES (256ll << 20)  // the window of the formatted text that is written and brought back at a time

namespace {

// text | index | sel | relabel_index | label_id | blob | sizes | prefix | status and head word (the uploaded form's first two only)
struct FormatStage {
    uint8_t *text; int64_t *idx, *sel, *ri; int32_t *lab; uint8_t *blob; int64_t *size, *prefix, *words;
    void layout(Carver &k, int64_t text_bytes, int64_t n_records, int64_t nsel, bool uploaded, bool has_sel, bool has_ri, bool has_lab)
    {
        if (uploaded) {
            k.take(text, align_up(text_bytes > 0 ? text_bytes : 1, 16));
            k.take(idx, (n_records > 0 ? n_records : 1) * MPB_IDX_COLS);
        }
        if (has_sel) k.take(sel, nsel);
        if (has_ri) k.take(ri, nsel);
        if (has_lab) k.take(lab, nsel);
        k.take(blob, FM_BLOB_BYTES);
        k.take(size, nsel);
        k.take(prefix, nsel + 1);
        k.take(words, 2);
    }
};

// one window of the text form, or the CRC ranges and refusal marks of one piece of the compressed form
struct FormatOut {
    uint8_t *out; mpb_crc_range *ranges; uint32_t *bad;
    void layout(Carver &k, int64_t window, int64_t members)
    {
        if (window > 0) k.take(out, align_up(window, 16));
        if (members > 0) { k.take(ranges, members); k.take(bad, members); }
    }
};

int str_len_ok(const char *s, const char *what, int64_t *len)
{
    const size_t n = strnlen(s, FM_STR_MAX + 1);
    if (n > FM_STR_MAX) return fail(MPB_E_INVALID, "mpb_format_text_host: %s is longer than %d bytes", what, FM_STR_MAX);
    *len = (int64_t)n;
    return MPB_OK;
}

}  // namespace

int mpb_format_text_host(mpb_ctx *c, const char *text, int64_t text_bytes, const int64_t *idx, int64_t n_records, int64_t resident,
                         const int64_t *sel, int64_t nsel, int32_t kind, int32_t fastq_offset, int32_t out_offset, int32_t clamp_q0,
                         int32_t max_len, const char *relabel, const int64_t *relabel_index, const char *const *labels,
                         int32_t n_labels, const int32_t *label_id, int32_t bgzf, uint8_t *out, int64_t out_cap, int64_t *out_bytes,
                         int64_t *text_needed, int64_t *bad_record, mpb_bgzf_stats *stats)
{
    // 1. the arguments: what is wrong with them is said with or without a device
    if (out_bytes) *out_bytes = 0;
    if (text_needed) *text_needed = 0;
    if (bad_record) *bad_record = -1;
    if (stats) memset(stats, 0, sizeof(*stats));
    const bool uploaded = resident == 0;
    if (!out_bytes || !text_needed || !bad_record || nsel < 0 || n_records < 0 || text_bytes < 0 || out_cap < 0 || (out_cap > 0 && !out))
        return fail(MPB_E_INVALID, "mpb_format_text_host: bad arguments (a NULL where a pointer is needed, or a negative size)");
    if (resident < 0) return fail(MPB_E_INVALID, "mpb_format_text_host: resident %lld is no generation", (long long)resident);
    if (uploaded ? (!idx || (text_bytes > 0 && !text)) : (text != nullptr || idx != nullptr))
        return fail(MPB_E_INVALID, "mpb_format_text_host: either text and idx (resident == 0) or the resident text's generation, not both or neither");
    if (kind != FM_KIND_FASTA && kind != FM_KIND_QUAL && kind != FM_KIND_FASTQ)
        return fail(MPB_E_INVALID, "mpb_format_text_host: kind %d is none of fasta (0), qual (1), fastq (2)", (int)kind);
    if (fastq_offset < 0 || fastq_offset > 255 || out_offset < 0 || out_offset > 255)
        return fail(MPB_E_INVALID, "mpb_format_text_host: fastq_offset %d / out_offset %d outside 0..255", (int)fastq_offset, (int)out_offset);
    if (relabel && !relabel_index) return fail(MPB_E_INVALID, "mpb_format_text_host: relabel without relabel_index");
    if (n_labels < 0 || n_labels > FM_MAX_LABELS)
        return fail(MPB_E_INVALID, "mpb_format_text_host: %d labels: at most %d", (int)n_labels, FM_MAX_LABELS);
    if (label_id && (!labels || n_labels == 0)) return fail(MPB_E_INVALID, "mpb_format_text_host: label_id without labels");
    if (max_len < 0) return fail(MPB_E_INVALID, "mpb_format_text_host: max_len %d is negative", (int)max_len);
    int rc;
    FmParams p;
    memset(&p, 0, sizeof(p));
    std::vector<uint8_t> blob;
    try { blob.assign(FM_BLOB_BYTES, 0); }
    catch (const std::bad_alloc &) { return fail(MPB_E_NOMEM, "out of host memory"); }
    int64_t len = 0;
    if (relabel) {
        if ((rc = str_len_ok(relabel, "relabel", &len))) return rc;
        memcpy(blob.data(), relabel, (size_t)len);
        p.str_len[0] = (uint8_t)len;
    }
    if (label_id)
        for (int i = 0; i < n_labels; i++) {
            if (!labels[i]) return fail(MPB_E_INVALID, "mpb_format_text_host: label %d is NULL", i);
            if ((rc = str_len_ok(labels[i], "a label", &len))) return rc;
            memcpy(blob.data() + (size_t)(1 + i) * FM_SLOT, labels[i], (size_t)len);
            p.str_len[1 + i] = (uint8_t)len;
        }
    if (uploaded && (rc = check_text_bytes(text_bytes))) return rc;
    p.n_records = n_records; p.text_bytes = text_bytes;
    p.kind = kind; p.fastq_offset = fastq_offset; p.out_offset = out_offset; p.floor_q = clamp_q0 ? 1 : 0; p.max_len = max_len;
    p.has_relabel = relabel ? 1 : 0; p.has_labels = label_id ? 1 : 0; p.n_labels = label_id ? n_labels : 0;
    // 2. the rows of an uploaded index, before anything goes up: the kernels' own checks, made here first
    if (uploaded)
        for (int64_t k = 0; k < nsel; k++) {
            FmRow r;
            if (!fm_row(idx, sel, relabel_index, label_id, k, p, &r)) {
                *bad_record = k;
                return fail(MPB_E_INVALID, "mpb_format_text_host: selected record %lld fails a check (sel, the row's offsets and lengths "
                            "against the text, relabel_index, label_id)", (long long)k);
            }
        }
    CTXCHK(c);
    if (!uploaded) {
        if (resident != c->resident.gen)
            return fail(MPB_E_INVALID, "mpb_format_text_host: text %lld is not resident (the context holds %lld; 0: none)",
                        (long long)resident, (long long)c->resident.gen);
        if (n_records != c->resident.n)
            return fail(MPB_E_INVALID, "mpb_format_text_host: n_records %lld is not the resident index's %lld", (long long)n_records,
                        (long long)c->resident.n);
        p.text_bytes = c->resident.text_bytes;
    }
    if (nsel == 0) return MPB_OK;
    // 3. the stage, the small uploads, count and prefix
    FormatStage st{};
    if ((rc = carve(c, c->format_stage, [&](Carver &k) {
            st.layout(k, text_bytes, n_records, nsel, uploaded, sel != nullptr, relabel != nullptr, label_id != nullptr); }))) return rc;
    const uint8_t *d_text = uploaded ? st.text : c->resident.text;
    const int64_t *d_idx = uploaded ? st.idx : c->resident.idx;
    hipStream_t s = c->stream;
    int64_t *words = c->pin->fmt_words;
    std::vector<int64_t> prefix;
    std::vector<mpb_crc_range> ranges;
    BgzfHost bh;
    StreamQueue q(c);                                        // (it leaves before the vectors above)
    if (uploaded) {
        q.up(st.text, text, text_bytes);
        q.up(st.idx, idx, n_records * MPB_IDX_COLS * (int64_t)sizeof(int64_t));
    }
    if (sel) q.up(st.sel, sel, nsel * (int64_t)sizeof(int64_t));
    if (relabel) q.up(st.ri, relabel_index, nsel * (int64_t)sizeof(int64_t));
    if (label_id) q.up(st.lab, label_id, nsel * (int64_t)sizeof(int32_t));
    q.up(st.blob, blob.data(), FM_BLOB_BYTES);
    words[0] = INT64_MAX; words[1] = 0;
    q.up(st.words, words, 2 * sizeof(int64_t));
    q.run(MPB_K_PACK_TEXT, [&] {
        mpb_launch_fmt_count(d_text, d_idx, st.sel, st.ri, st.lab, nsel, p, st.size, st.prefix, st.words + 1, st.words, s); });
    q.down(words, st.words, 2 * sizeof(int64_t));
    if ((rc = q.wait("hipMemcpyAsync (format uploads) / k_fmt_count / k_fmt_scan"))) return rc;
    if (words[0] != INT64_MAX) {
        *bad_record = words[0];
        return fail(MPB_E_INVALID, "mpb_format_text_host: the kernel refused selected record %lld%s", (long long)words[0],
                    uploaded ? "" : " of the resident index (never expected)");
    }
    const int64_t total = words[1];
    if (total < 0) return fail(MPB_E_HIP, "mpb_format_text_host: k_fmt_scan's total is %lld (never expected)", (long long)total);
    *text_needed = total;
    // 4. the sizes
    if (!bgzf && out_cap < total)
        return fail(MPB_E_INVALID, "mpb_format_text_host: out_cap %lld is too small: the formatted text has %lld bytes", (long long)out_cap,
                    (long long)total);
    if (bgzf) {
        int64_t bound = 0;
        if ((rc = mpb_bgzf_bound(total, &bound))) return rc;
        if (out_cap < bound)
            return fail(MPB_E_INVALID, "mpb_format_text_host: out_cap %lld is below mpb_bgzf_bound's %lld for the %lld bytes of formatted text",
                        (long long)out_cap, (long long)bound, (long long)total);
    }
    // 5. windows of the formatted text, one after the other: the records that reach into a window are written clipped to it, so
    // a window's edges need not be records' edges and -- the compressed form -- members are cut from the whole text
    int64_t limit = env_int64("MPB_FORMAT_PIECE_BYTES", 1, MPB_FORMAT_PIECE_BYTES - 1, MPB_FORMAT_PIECE_BYTES);
    const int64_t members = (total + MPB_BGZF_DATA - 1) / MPB_BGZF_DATA;
    int64_t per_piece = 0;
    if (bgzf) {
        per_piece = std::min(bgzf_piece_members(members), std::max<int64_t>(1, limit / MPB_BGZF_DATA));
        limit = per_piece * (int64_t)MPB_BGZF_DATA;
    }
    const int64_t window = std::min(limit, total);
    if (total > window) {                                    // more than one window: the prefix says which records reach into which
        try { prefix.resize((size_t)nsel + 1); }
        catch (const std::bad_alloc &) { return fail(MPB_E_NOMEM, "out of host memory for %lld prefix words", (long long)nsel + 1); }
        q.down(prefix.data(), st.prefix, (nsel + 1) * (int64_t)sizeof(int64_t));
        if ((rc = q.wait("hipMemcpyAsync (format prefix)"))) return rc;
        if (prefix[0] != 0 || prefix[(size_t)nsel] != total || !std::is_sorted(prefix.begin(), prefix.end()))
            return fail(MPB_E_HIP, "mpb_format_text_host: k_fmt_scan's prefix is not one (never expected)");
    }
    FormatOut fo{};
    BgzfStage bst{};
    if ((rc = carve(c, c->format_out, [&](Carver &k) { fo.layout(k, bgzf ? 0 : window, per_piece); }))) return rc;
    if (bgzf) {
        if ((rc = bh.reserve(per_piece))) return rc;
        try { ranges.resize((size_t)per_piece); }
        catch (const std::bad_alloc &) { return fail(MPB_E_NOMEM, "out of host memory for %lld members", (long long)per_piece); }
        if ((rc = carve(c, c->bgzf_stage, [&](Carver &k) { bst.layout(k, per_piece); }))) return rc;
    }
    int64_t written = 0;
    for (int64_t lo = 0; lo < total; lo += window) {
        const int64_t hi = std::min(lo + window, total);
        int64_t k0 = 0, k1 = nsel;
        if (!prefix.empty()) {
            k0 = (std::upper_bound(prefix.begin(), prefix.begin() + nsel, lo) - prefix.begin()) - 1;
            k1 = std::lower_bound(prefix.begin(), prefix.begin() + nsel, hi) - prefix.begin();
        }
        uint8_t *d_out = bgzf ? bst.text : fo.out;
        q.run(MPB_K_PACK_TEXT, [&] {
            mpb_launch_fmt_write(d_text, st.blob, d_idx, st.sel, st.ri, st.lab, k0, k1, p, st.prefix, st.words, lo, hi, d_out, s); });
        if (!bgzf) {                                         // (the next window's kernel runs behind this copy: one wait at the end)
            q.down(out + lo, fo.out, hi - lo);
            written = hi;
            continue;
        }
        const int64_t tb = hi - lo, nm = (tb + MPB_BGZF_DATA - 1) / MPB_BGZF_DATA;
        for (int64_t m = 0; m < nm; m++)
            ranges[(size_t)m] = mpb_crc_range{m * (int64_t)MPB_BGZF_DATA, (int32_t)std::min<int64_t>(MPB_BGZF_DATA, tb - m * (int64_t)MPB_BGZF_DATA), 0};
        q.up(fo.ranges, ranges.data(), nm * (int64_t)sizeof(mpb_crc_range));
        int64_t got = 0;
        if ((rc = bgzf_compress_piece(q, bst, tb, nm, nullptr, fo.ranges, fo.bad, bh, out + written, out_cap - written, &got, stats)))
            return rc;
        written += got;
    }
    if ((rc = q.wait("k_fmt_write / hipMemcpyAsync (formatted text)"))) return rc;
    *out_bytes = written;
    return MPB_OK;
}
