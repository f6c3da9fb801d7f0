// mpb_format.cpp -- the writer's formatter on the device, behind the C ABI of libmoira_pb.so (include/moira_pb.h): the entries that
// turn selected records of a text and its record index into fasta, qual or fastq text (mpb_format_text_host) and, beyond that,
// into contigs.report lines, with the ";ee=..;size=1;" suffix where asked for (mpb_format_records_host), from an upload
// or from what the last filter call left on the device (the resident form), and hands back the text or -- compressed where it
// lies by mpb_bgzf.cpp's piece -- its BGZF members.  The kernels are mpb_format_kernels.hip (k_fmt_count, k_fmt_scan, k_fmt_write,
// inside MPB_K_PACK_TEXT's span: they have no id of their own); what a lane does, and the row checks the host makes first, are
// mpb_format_lane.inc.  mio_format and mio_format_report (csrc/fastio.cpp) define the output.  The entry queues on one StreamQueue (mpb_queue.h).
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
#define FM_LD_U64(p, k) fm_hload_u64((p), (k))
static inline uint64_t fm_hload_u64(const uint64_t *p, int64_t k)      // (the caller's doubles, read as bytes)
{
    uint64_t v;
    memcpy(&v, (const char *)p + 8 * k, 8);
    return v;
}
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
    uint8_t *text; int64_t *idx, *sel, *ri; int32_t *lab; uint8_t *blob; int64_t *size, *prefix, *words; uint64_t *ee; int32_t *aux;
    void layout(Carver &k, int64_t text_bytes, int64_t n_records, int64_t nsel, bool uploaded, bool has_sel, bool has_ri, bool has_lab,
                bool has_ee, bool has_aux)
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
        if (has_ee) k.take(ee, nsel);
        if (has_aux) k.take(aux, (n_records > 0 ? n_records : 1) * 3);
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

int str_len_ok(const char *who, const char *s, const char *what, int64_t *len)
{
    const size_t n = strnlen(s, FM_STR_MAX + 1);
    if (n > FM_STR_MAX) return fail(MPB_E_INVALID, "%s: %s is longer than %d bytes", who, what, FM_STR_MAX);
    *len = (int64_t)n;
    return MPB_OK;
}

// both entries; who: the entry's name for its messages; records: mpb_format_records_host (the report kind is taken)
int format_records(const char *who, bool records, mpb_ctx *c, const char *text, int64_t text_bytes, const int64_t *idx, int64_t n_records,
                   int64_t resident, const int64_t *sel, int64_t nsel, int32_t kind, int32_t fastq_offset, int32_t out_offset,
                   int32_t clamp_q0, int32_t max_len, const char *relabel, const int64_t *relabel_index, const char *const *labels,
                   int32_t n_labels, const int32_t *label_id, const double *ee, const int32_t *aux, int32_t bgzf, uint8_t *out,
                   int64_t out_cap, int64_t *out_bytes, int64_t *text_needed, int64_t *bad_record, mpb_bgzf_stats *stats)
{
    // 1. the arguments: what is wrong with them is said with or without a device
    if (out_bytes) *out_bytes = 0;
    if (text_needed) *text_needed = 0;
    if (bad_record) *bad_record = -1;
    if (stats) memset(stats, 0, sizeof(*stats));
    const bool uploaded = resident == 0;
    if (!out_bytes || !text_needed || !bad_record || nsel < 0 || n_records < 0 || text_bytes < 0 || out_cap < 0 || (out_cap > 0 && !out))
        return fail(MPB_E_INVALID, "%s: bad arguments (a NULL where a pointer is needed, or a negative size)", who);
    if (resident < 0) return fail(MPB_E_INVALID, "%s: resident %lld is no generation", who, (long long)resident);
    if (uploaded ? (!idx || (text_bytes > 0 && !text)) : (text != nullptr || idx != nullptr))
        return fail(MPB_E_INVALID, "%s: either text and idx (resident == 0) or the resident text's generation, not both or neither", who);
    const bool report = records && kind == FM_KIND_REPORT;
    if (kind != FM_KIND_FASTA && kind != FM_KIND_QUAL && kind != FM_KIND_FASTQ && !report)
        return fail(MPB_E_INVALID, "%s: kind %d is none of fasta (0), qual (1), fastq (2)%s", who, (int)kind, records ? ", report (4)" : "");
    if (report && (labels || label_id)) return fail(MPB_E_INVALID, "%s: a report line (kind 4) takes no labels", who);
    if (report && uploaded && !aux) return fail(MPB_E_INVALID, "%s: a report line (kind 4) needs aux[n_records][3]", who);
    if (!report && aux) return fail(MPB_E_INVALID, "%s: aux goes with kind 4 alone", who);
    if (report && !uploaded && aux)
        return fail(MPB_E_INVALID, "%s: aux with a generation: the report lines of a generation are written from the arrays it carries", who);
    if (fastq_offset < 0 || fastq_offset > 255 || out_offset < 0 || out_offset > 255)
        return fail(MPB_E_INVALID, "%s: fastq_offset %d / out_offset %d outside 0..255", who, (int)fastq_offset, (int)out_offset);
    if (relabel && !relabel_index) return fail(MPB_E_INVALID, "%s: relabel without relabel_index", who);
    if (n_labels < 0 || n_labels > FM_MAX_LABELS)
        return fail(MPB_E_INVALID, "%s: %d labels: at most %d", who, (int)n_labels, FM_MAX_LABELS);
    if (label_id && (!labels || n_labels == 0)) return fail(MPB_E_INVALID, "%s: label_id without labels", who);
    if (max_len < 0) return fail(MPB_E_INVALID, "%s: max_len %d is negative", who, (int)max_len);
    int rc;
    FmParams p;
    memset(&p, 0, sizeof(p));
    std::vector<uint8_t> blob;
    try { blob.assign(FM_BLOB_BYTES, 0); }
    catch (const std::bad_alloc &) { return fail(MPB_E_NOMEM, "out of host memory"); }
    int64_t len = 0;
    if (relabel) {
        if ((rc = str_len_ok(who, relabel, "relabel", &len))) return rc;
        memcpy(blob.data(), relabel, (size_t)len);
        p.str_len[0] = (uint8_t)len;
    }
    if (label_id)
        for (int i = 0; i < n_labels; i++) {
            if (!labels[i]) return fail(MPB_E_INVALID, "%s: label %d is NULL", who, i);
            if ((rc = str_len_ok(who, labels[i], "a label", &len))) return rc;
            memcpy(blob.data() + (size_t)(1 + i) * FM_SLOT, labels[i], (size_t)len);
            p.str_len[1 + i] = (uint8_t)len;
        }
    if (uploaded && (rc = check_text_bytes(text_bytes))) return rc;
    p.n_records = n_records; p.text_bytes = text_bytes;
    p.kind = kind; p.fastq_offset = fastq_offset; p.out_offset = out_offset; p.floor_q = clamp_q0 ? 1 : 0; p.max_len = max_len;
    p.has_relabel = relabel ? 1 : 0; p.has_labels = label_id ? 1 : 0; p.n_labels = label_id ? n_labels : 0;
    p.has_ee = ee ? 1 : 0; p.aux_stride = 3;
    const uint64_t *ee_bits = (const uint64_t *)ee;
    const int32_t *const h_aux[3] = {aux, aux ? aux + 1 : nullptr, aux ? aux + 2 : nullptr};
    // 2. before anything goes up, the first selected record that cannot be taken: its ee ("%.2f" is rendered on the device for
    // finite values below 2^53 alone; either form: ee always comes from the host), or -- an uploaded index -- its row: the kernels'
    // own checks, made here first
    for (int64_t k = 0; k < nsel && (ee || uploaded); k++) {
        uint64_t q;
        int32_t neg;
        if (ee && !fm_ee_q(fm_hload_u64(ee_bits, k), &q, &neg)) {
            *bad_record = k;
            return fail(MPB_E_INVALID, "%s: ee[%lld] = %g is outside what the device renders (finite, |ee| < 2^53)", who, (long long)k, ee[k]);
        }
        FmRow r;
        FmExtra x;
        if (uploaded && !fm_rec_row(idx, sel, relabel_index, label_id, ee_bits, h_aux[0], h_aux[1], h_aux[2], k, p, &r, &x)) {
            *bad_record = k;
            return fail(MPB_E_INVALID, "%s: selected record %lld fails a check (sel, the row's offsets and lengths "
                        "against the text, relabel_index, label_id)", who, (long long)k);
        }
    }
    CTXCHK(c);
    if (!uploaded) {
        if (resident != c->resident.gen)
            return fail(MPB_E_INVALID, "%s: text %lld is not resident (the context holds %lld; 0: none)", who,
                        (long long)resident, (long long)c->resident.gen);
        if (n_records != c->resident.n)
            return fail(MPB_E_INVALID, "%s: n_records %lld is not the resident index's %lld", who, (long long)n_records,
                        (long long)c->resident.n);
        if (report && !c->resident.aux[0])
            return fail(MPB_E_INVALID, "%s: generation %lld carries no aux: only the contigs of mpb_contigs_filter_fastq_host have report lines",
                        who, (long long)resident);
        p.text_bytes = c->resident.text_bytes;
        p.aux_stride = 1;
    }
    if (nsel == 0) return MPB_OK;
    // 3. the stage, the small uploads, count and prefix
    FormatStage st{};
    if ((rc = carve(c, c->format_stage, [&](Carver &k) {
            st.layout(k, text_bytes, n_records, nsel, uploaded, sel != nullptr, relabel != nullptr, label_id != nullptr, ee != nullptr,
                      report && uploaded); }))) return rc;
    const int32_t *d_aux[3] = {nullptr, nullptr, nullptr};
    for (int j = 0; j < 3 && report; j++) d_aux[j] = uploaded ? st.aux + j : c->resident.aux[j];
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
    if (ee) q.up(st.ee, ee, nsel * (int64_t)sizeof(double));
    if (report && uploaded && n_records > 0) q.up(st.aux, aux, n_records * 3 * (int64_t)sizeof(int32_t));
    q.up(st.blob, blob.data(), FM_BLOB_BYTES);
    words[0] = INT64_MAX; words[1] = 0;
    q.up(st.words, words, 2 * sizeof(int64_t));
    q.run(MPB_K_PACK_TEXT, [&] {
        mpb_launch_fmt_count(d_text, d_idx, st.sel, st.ri, st.lab, st.ee, d_aux, nsel, p, st.size, st.prefix, st.words + 1, st.words, s); });
    q.down(words, st.words, 2 * sizeof(int64_t));
    if ((rc = q.wait("hipMemcpyAsync (format uploads) / k_fmt_count / k_fmt_scan"))) return rc;
    if (words[0] != INT64_MAX) {
        *bad_record = words[0];
        return fail(MPB_E_INVALID, "%s: the kernel refused selected record %lld%s", who, (long long)words[0],
                    uploaded ? "" : " of the resident index (never expected)");
    }
    const int64_t total = words[1];
    if (total < 0) return fail(MPB_E_HIP, "%s: k_fmt_scan's total is %lld (never expected)", who, (long long)total);
    *text_needed = total;
    // 4. the sizes
    if (!bgzf && out_cap < total)
        return fail(MPB_E_INVALID, "%s: out_cap %lld is too small: the formatted text has %lld bytes", who, (long long)out_cap,
                    (long long)total);
    if (bgzf) {
        int64_t bound = 0;
        if ((rc = mpb_bgzf_bound(total, &bound))) return rc;
        if (out_cap < bound)
            return fail(MPB_E_INVALID, "%s: out_cap %lld is below mpb_bgzf_bound's %lld for the %lld bytes of formatted text", who,
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
            return fail(MPB_E_HIP, "%s: k_fmt_scan's prefix is not one (never expected)", who);
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
            mpb_launch_fmt_write(d_text, st.blob, d_idx, st.sel, st.ri, st.lab, st.ee, d_aux, k0, k1, p, st.prefix, st.words, lo, hi, d_out, s); });
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

}  // namespace

int mpb_format_text_host(mpb_ctx *c, const char *text, int64_t text_bytes, const int64_t *idx, int64_t n_records, int64_t resident,
                         const int64_t *sel, int64_t nsel, int32_t kind, int32_t fastq_offset, int32_t out_offset, int32_t clamp_q0,
                         int32_t max_len, const char *relabel, const int64_t *relabel_index, const char *const *labels,
                         int32_t n_labels, const int32_t *label_id, int32_t bgzf, uint8_t *out, int64_t out_cap, int64_t *out_bytes,
                         int64_t *text_needed, int64_t *bad_record, mpb_bgzf_stats *stats)
{
    return format_records("mpb_format_text_host", false, c, text, text_bytes, idx, n_records, resident, sel, nsel, kind, fastq_offset,
                          out_offset, clamp_q0, max_len, relabel, relabel_index, labels, n_labels, label_id, nullptr, nullptr, bgzf, out,
                          out_cap, out_bytes, text_needed, bad_record, stats);
}

int mpb_format_records_host(mpb_ctx *c, const char *text, int64_t text_bytes, const int64_t *idx, int64_t n_records, int64_t resident,
                            const int64_t *sel, int64_t nsel, int32_t kind, int32_t fastq_offset, int32_t out_offset, int32_t clamp_q0,
                            int32_t max_len, const char *relabel, const int64_t *relabel_index, const char *const *labels,
                            int32_t n_labels, const int32_t *label_id, const double *ee, const int32_t *aux, int32_t bgzf, uint8_t *out,
                            int64_t out_cap, int64_t *out_bytes, int64_t *text_needed, int64_t *bad_record, mpb_bgzf_stats *stats)
{
    return format_records("mpb_format_records_host", true, c, text, text_bytes, idx, n_records, resident, sel, nsel, kind, fastq_offset,
                          out_offset, clamp_q0, max_len, relabel, relabel_index, labels, n_labels, label_id, ee, aux, bgzf, out, out_cap,
                          out_bytes, text_needed, bad_record, stats);
}
