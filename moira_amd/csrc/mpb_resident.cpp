// mpb_resident.cpp -- the resident path of the C ABI of libmoira_pb.so (include/moira_pb.h): batches that already lie in device
// memory.  Argument validation with the reference's error behaviour (moira/bernoullimodule.c:79-90), the launch sequence of the
// sorted pipeline and of the natural-order narrow pass, the choice between them, the queries about the last call, the
// classified-at-source pair, text decode / encode and the synthetic fill.  Every result comes from the HIP kernels.
// (Every mpb_* function defined here has C linkage: include/moira_pb.h declares it inside extern "C".)

#include "mpb_ctx.h"

#include <cmath>
#include <cstdlib>
#include <cstring>

// ---- the hot path --------------------------------------------------------------------------------

MpbDevParams make_dev_params(const mpb_filter_params *p, int32_t fixed_len, int32_t max_len)
{
    MpbDevParams d;
    d.thr = 1 - p->alpha;                     // same double expression as the reference
    d.uncert = p->uncert;
    d.maxerrors = p->maxerrors;
    const double z = inv_norm_cdf(1 - p->alpha);
    d.z = (float)z;
    d.zq = (float)((z * z - 1) / 6);
    // alpha below half an ulp of 1: 1 - alpha == 1 and Phi^-1 is inf / inf.  The prediction there is "every row" (no read crosses
    // before its last one); say so with finite constants instead of leaving it to what fminf makes of a NaN in the kernels.
    if (!(z == z) || std::isinf(z)) { d.z = 1e30f; d.zq = 0.0f; }
    d.clow = (float)(sqrt(2 * log(1 / (1 - p->alpha))) * 1.0001);
    d.ambig_mode = p->ambig_mode;
    d.flags = p->flags;
    d.fixed_len = fixed_len;
    d.max_len = max_len;
    d.len_shift = MPB_LEN_SHIFT;
    while (((max_len - 1) >> d.len_shift) >= MPB_LEN_BINS) d.len_shift++;
    return d;
}

// argument checks shared by mpb_filter_device and the classified-at-source pair; *max_len_out = longest read the batch can hold
static int check_device_batch(const void *d_q, int64_t n, int64_t row_stride, const int32_t *d_len, int32_t fixed_len,
                              const void *d_ee, const void *d_ns, const void *d_pass, int32_t *max_len_out)
{
    if (n < 0) return fail(MPB_E_INVALID, "n < 0");
    if (n > 0x7fffffffll - 4096) return fail(MPB_E_INVALID, "batch of %lld reads exceeds 2^31; split it", (long long)n);
    if (row_stride <= 0 || row_stride % 16 != 0) return fail(MPB_E_INVALID, "row_stride must be a positive multiple of 16");
    if (row_stride > MPB_MAX_STRIDE) return fail(MPB_E_INVALID, "row_stride %lld exceeds %d (reads longer than %d bases are not supported)", (long long)row_stride, MPB_MAX_STRIDE, MPB_MAX_LEN);
    if (((uintptr_t)d_q & 15) != 0) return fail(MPB_E_INVALID, "quality matrix must be 16-byte aligned");
    if (!d_len && (fixed_len < 0 || fixed_len > row_stride)) return fail(MPB_E_INVALID, "fixed_len %d does not fit row_stride %lld", fixed_len, (long long)row_stride);
    const int32_t max_len = d_len ? (int32_t)(row_stride < MPB_MAX_LEN ? row_stride : MPB_MAX_LEN) : fixed_len;
    if (max_len > MPB_MAX_LEN)
        return fail(MPB_E_INVALID, "reads longer than %d bases are not supported", MPB_MAX_LEN);
    if (n > 0 && (!d_q || !d_ee || !d_ns || !d_pass)) return fail(MPB_E_INVALID, "NULL device buffer");
    *max_len_out = max_len;
    return MPB_OK;
}

// workspace (and, for batches whose rows can hold reads of more than 1023 bases, the wide-read list) of a batch of n reads
static int prepare_batch(mpb_ctx *c, int64_t n, int32_t max_len)
{
    int rc = ensure_workspace(c, n);
    if (rc) return rc;
    // reads of more than 1023 bases may need more DP rows than one wave holds: such reads are listed by the prepass
    // and run by the wide kernel (k_wide).  Batches whose rows cannot hold such a read never see any of it.
    if (max_len + 1 > MPB_TILE_MAX_ROWS) {
        if ((rc = ensure_wide_workspace(c, n))) return rc;
        HIPCHK(hipMemsetAsync(c->ws.wide_count, 0, sizeof(int32_t), c->stream));
    }
    return MPB_OK;
}

// The counts of a batch, through the pinned words: passes, overflow re-runs (sorted: the sorted pipeline ran, k_tables zeroed the
// pass counter) and bad lengths, which fail the call (raised by this call or an earlier one that fetched no counts: moira_pb.h;
// the prepass gave those reads ee = NaN, pass = 0, never a result computed on a clamped length).
static int fetch_counts(mpb_ctx *c, int64_t n, int64_t row_stride, const int32_t *d_len, int32_t max_len, const uint8_t *d_pass,
                        bool sorted, mpb_filter_counts *counts)
{
    hipStream_t s = c->stream;
    unsigned long long *np = &c->pin->n_pass;
    int32_t *novf = &c->pin->n_overflow, *bad = &c->pin->bad_len;
    *novf = *bad = 0;
    if (!sorted) HIPCHK(hipMemsetAsync(c->ws.pass_count, 0, sizeof(unsigned long long), s));
    mpb_launch_count(d_pass, n, c->ws, s);
    HIPCHK(hipMemcpyAsync(np, c->ws.pass_count, sizeof(*np), hipMemcpyDeviceToHost, s));
    if (sorted) HIPCHK(hipMemcpyAsync(novf, c->ws.ovf_count, sizeof(*novf), hipMemcpyDeviceToHost, s));
    if (d_len) HIPCHK(hipMemcpyAsync(bad, c->ws.bad_len, sizeof(*bad), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (*bad) {
        HIPCHK(hipMemsetAsync(c->ws.bad_len, 0, sizeof(int32_t), s));
        return fail(MPB_E_INVALID, "%d read length(s) in d_len outside 0..%d (row_stride %lld; reads longer than %d bases "
                    "are not supported); those reads were given ee = NaN, pass = 0", *bad, max_len, (long long)row_stride, MPB_MAX_LEN);
    }
    counts->n_pass = (int64_t)*np;
    counts->n_fail = n - (int64_t)*np;
    counts->n_overflow = *novf;
    return MPB_OK;
}

// everything after the classification: scan -> scatter -> DP -> wide reads -> overflow pass (-> counts)
static int filter_device_tail(mpb_ctx *c, const uint8_t *d_q, int64_t n, int64_t row_stride, const int32_t *d_len,
                              const MpbDevParams &prm, double *d_ee, int32_t *d_ns, uint8_t *d_pass, mpb_filter_counts *counts,
                              const int32_t *d_list = nullptr)
{
    hipStream_t s = c->stream;
    const int32_t max_len = prm.max_len;
    { Span t(c, MPB_K_SCAN);     mpb_launch_scan(n, d_len, c->ws, s); }
    { Span t(c, MPB_K_SCATTER);  mpb_launch_scatter(n, d_len, d_ns, prm, c->ws, s, d_list); }
    // MPB_FLAG_ODDS: the main pass alone, and only on the context's own table (a private one -- scores above 254 -- has no odds twin)
    const double2 *lut_odds = (prm.flags & MPB_FLAG_ODDS) && c->ws.lut == c->d_lut ? c->d_lut_odds : nullptr;
    { Span t(c, MPB_K_DP);       mpb_launch_dp(d_q, n, row_stride, d_len, prm, c->ws, d_ns, d_ee, d_pass, s, lut_odds); }
    if (max_len + 1 > MPB_TILE_MAX_ROWS) { Span t(c, MPB_K_WIDE); mpb_launch_wide(d_q, row_stride, d_len, prm, c->ws, d_ns, d_ee, d_pass, s); }
    { Span t(c, MPB_K_OVERFLOW); mpb_launch_overflow(d_q, n, row_stride, d_len, prm, c->ws, d_ns, d_ee, d_pass, s); }
    HIPCHK(hipGetLastError());
    return counts ? fetch_counts(c, n, row_stride, d_len, max_len, d_pass, true, counts) : MPB_OK;
}

// Fixed-length batches, and (round 6) ragged ones whose rows hold up to MPB_RG_MAX_STRIDE bytes (k_narrow_rg).
static bool narrow_eligible(const mpb_ctx *c, int64_t n, int64_t row_stride, const int32_t *d_len, int32_t fixed_len, const mpb_filter_params *p)
{
    uint32_t forbidden = MPB_FLAG_FAST_FMA | MPB_FLAG_ODDS | MPB_FLAG_TEST_UNDERPREDICT | MPB_FLAG_DECISION_ONLY | MPB_FLAG_COUNT_CELLS | MPB_FLAG_NO_NARROW;
    if (p->flags & MPB_FLAG_ODDS_NARROW) forbidden &= ~MPB_FLAG_ODDS;      // the pass has a one-FMA form (check_params: the flag implies MPB_FLAG_ODDS)
    if (!(c->narrow_ok && n >= 1 && !(p->flags & forbidden) && c->ws.lut == c->d_lut)) return false;
    return d_len ? row_stride <= MPB_RG_MAX_STRIDE : fixed_len >= 1;
}

// d_list != nullptr: the sorted pipeline over the n reads d_list[0 .. n) of a matrix of n_matrix reads (the reads a narrow pass hands
// back), where they lie: rows, lengths, class bytes and results are addressed by read (so the workspace is sized for the matrix: about
// 12 bytes per read, what the sorted pipeline would have taken for the same batch), the permutation by position; counts must be NULL.
static int filter_device_general(mpb_ctx *c, const uint8_t *d_q, int64_t n, int64_t row_stride, const int32_t *d_len,
                                 int32_t fixed_len, int32_t max_len, const mpb_filter_params *params,
                                 double *d_ee, int32_t *d_ns, uint8_t *d_pass, mpb_filter_counts *counts,
                                 const int32_t *d_list = nullptr, int64_t n_matrix = 0)
{
    int rc;
    if ((rc = prepare_batch(c, d_list && n_matrix > n ? n_matrix : n, max_len))) return rc;
    const MpbDevParams prm = make_dev_params(params, fixed_len, max_len);
    if (params->flags & MPB_FLAG_COUNT_CELLS) HIPCHK(hipMemsetAsync(c->ws.alg_cells, 0, sizeof(unsigned long long), c->stream));
    { Span t(c, MPB_K_PREPASS);  mpb_launch_prepass(d_q, n, row_stride, d_len, prm, c->ws, d_ns, d_ee, d_pass, c->stream, d_list); }
    return filter_device_tail(c, d_q, n, row_stride, d_len, prm, d_ee, d_ns, d_pass, counts, d_list);
}

// 0: the sorted pipeline; 2..4: the narrow pass with that many rows.  May draw a sample (one small launch + a synchronisation).
// *split (ragged batches, *rows0 >= 3): groups whose longest read has at most that many 16-byte chunks run with a row less (0: none)
static int narrow_choose(mpb_ctx *c, const uint8_t *d_q, int64_t n, int64_t row_stride, const int32_t *d_len, int32_t fixed_len,
                         const mpb_filter_params *params, const MpbDevParams &prm, int *rows0, int *split)
{
    *rows0 = 0;
    *split = 0;
    c->last_path.sampled = 0;
    const int forced = (int)((params->flags >> 8) & 15u);
    if (forced) {
        *rows0 = forced < MPB_NAR_MIN_ROWS ? MPB_NAR_MIN_ROWS : forced > MPB_NAR_MAX_ROWS ? MPB_NAR_MAX_ROWS : forced;
        *split = d_len && !(params->flags & MPB_FLAG_ODDS_NARROW) ? (int)((params->flags >> 12) & 255u) : 0;   // MPB_FLAG_NARROW_SPLIT (test / measurement hook)
        return MPB_OK;
    }
    if (n < MPB_NAR_AUTO_MIN_READS) return MPB_OK;
    auto &ch = c->nar_choice;
    if (d_len) fixed_len = -1;                                // (a ragged batch of the same shape is another batch)
    const bool same = ch.valid && ch.n == n && ch.stride == row_stride && ch.fixed_len == fixed_len &&
                      memcmp(&ch.alpha, &params->alpha, sizeof(double)) == 0 && ch.flags == params->flags;
    if (same && ch.calls < 64) { ch.calls++; *rows0 = ch.rows0; *split = ch.split; return MPB_OK; }
    // a sample of <= 0.1 % of the reads: the prepass' row prediction on 256 .. 4096 reads spread over the batch
    int n_sample = (int)(n / 1024 < 256 ? 256 : n / 1024 > 4096 ? 4096 : n / 1024);
    { Span t(c, MPB_K_SAMPLE); mpb_launch_sample(d_q, n, row_stride, fixed_len, d_len, prm, c->ws, n_sample, c->stream); }
    HIPCHK(hipMemcpyAsync(c->pin->sample, c->ws.nar_sample, sizeof(c->pin->sample), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->last_path.sampled = 1;
    const int32_t *sample = c->pin->sample;
    int weight = 0;                                           // reads, or (ragged batches) their 16-byte chunks
    for (int k = 0; k < MPB_NAR_BUCKETS; k++) { c->last_path.sample_hist[k] = sample[k]; weight += sample[k]; }
    const bool odds = (params->flags & MPB_FLAG_ODDS_NARROW) != 0;
    *rows0 = narrow_rows_from_sample(sample, weight, odds);
    if (d_len && *rows0 >= 3 && !odds) {
        // mixed rows: the shortest sampled read that needs rows0 rows has `need` chunks; groups safely below it take a row less
        // (a sixteenth of margin and a chunk -- a cut that turns out too bold is dropped after the call that shows it, below; not
        // worth a second code path below four chunks)
        const int need = sample[MPB_NAR_BUCKETS + (*rows0 - 3)];
        if (need > 0 && need < (1 << 20)) {
            const int cut = need - 1 - need / 16;
            if (cut >= 4) *split = cut > 255 ? 255 : cut;
        }
    }
    ch.split = *split;
    {
        double back = sample[0];
        for (int r = *rows0 + 1; r < MPB_NAR_BUCKETS; r++) back += sample[r];
        ch.expect_back = weight > 0 ? back / weight : 0.0;
    }
    ch.valid = true; ch.n = n; ch.stride = row_stride; ch.fixed_len = fixed_len; ch.alpha = params->alpha; ch.flags = params->flags;
    ch.rows0 = *rows0; ch.calls = 0;
    return MPB_OK;
}

// MPB_NARROW_GRID_BLOCKS (include/moira_pb.h, a test hook): a cap on the workgroups of the pass' persistent grid, read per call;
// 0: none (unset, or anything but 1 .. MPB_NAR_GRID_CAP_MAX)
static int narrow_grid_cap()
{
    const char *e = getenv("MPB_NARROW_GRID_BLOCKS");
    if (!e || !*e) return 0;
    char *end = nullptr;
    const long v = strtol(e, &end, 10);
    return *end == 0 && v >= 1 && v <= MPB_NAR_GRID_CAP_MAX ? (int)v : 0;
}

static int filter_device_narrow(mpb_ctx *c, int rows0, int split, const uint8_t *d_q, int64_t n, int64_t row_stride, const int32_t *d_len,
                                int32_t fixed_len, const mpb_filter_params *params, const MpbDevParams &prm,
                                double *d_ee, int32_t *d_ns, uint8_t *d_pass, mpb_filter_counts *counts)
{
    int rc;
    hipStream_t s = c->stream;
    if ((rc = ensure_narrow_workspace(c, n, d_len != nullptr))) return rc;
    const int grid_cap = narrow_grid_cap();
    int nwaves = 0;
    { Span t(c, MPB_K_NARROW);
      mpb_launch_narrow(rows0, split, d_q, n, row_stride, fixed_len, d_len, prm, c->ws, d_ee, d_ns, d_pass, c->n_cu > 0 ? c->n_cu : 256,
                        c->rg_per_cu, grid_cap, &nwaves, s, (params->flags & MPB_FLAG_ODDS_NARROW) ? c->d_lut_odds : nullptr); }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(&c->pin->nar_count, c->ws.nar_count, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    const int64_t m = c->pin->nar_count;
    c->last_path.narrow_rows = rows0;
    c->last_path.narrow_waves = nwaves;
    c->last_path.narrow_split = d_len && rows0 >= 3 ? split : 0;
    c->last_path.n_fallback = m;
    const bool forced = ((params->flags >> 8) & 15u) != 0;
    // a pass that hands back far more than its sample can have promised: look again next time
    if (!forced && m > n / 2) c->nar_choice.valid = false;
    // mixed rows whose cut was too bold (reads of the short groups needed the row they did not get -- the sample's shortest such read
    // was not the batch's -- so that clearly more came back than the sample's own share of unfinished reads): the next calls of this
    // shape run without a cut
    if (!forced && split > 0 && (double)m > (1.5 * c->nar_choice.expect_back + 0.002) * (double)n) c->nar_choice.split = 0;
    c->classes_whole = false;                        // the class workspace: the handed-back reads at most
    if (m > 0) {
        // The reads handed back go through the sorted pipeline WHERE THEY LIE (round 6: the prepass and the scatter walk the list,
        // the DP addresses rows and results by read anyway): no dense copy of their rows, no block of memory for it.  When they
        // are most of the batch (a stale choice met a batch of bad reads) the whole batch takes the sorted pipeline instead:
        // the same results, one pass over everything is cheaper than a list of most of it (break-even near one half).
        if (!forced && m > n / 2) {
            c->last_path.n_fallback = n;
            c->classes_whole = true;
            return filter_device_general(c, d_q, n, row_stride, d_len, fixed_len, prm.max_len, params, d_ee, d_ns, d_pass, counts);
        }
        mpb_filter_params sub = *params;
        // (MPB_FLAG_ODDS stays: reads that only needed more rows get k_dp_odds, the ones the mode does not vouch for its overflow pass)
        sub.flags = (sub.flags & ~((15u << 8) | (255u << 12) | MPB_FLAG_ODDS_NARROW)) | MPB_FLAG_NO_NARROW;
        if ((rc = filter_device_general(c, d_q, m, row_stride, d_len, fixed_len, prm.max_len, &sub, d_ee, d_ns, d_pass, nullptr, c->ws.nar_list, n))) return rc;
        HIPCHK(hipGetLastError());
    }
    return counts ? fetch_counts(c, n, row_stride, d_len, prm.max_len, d_pass, m > 0, counts) : MPB_OK;
}

int mpb_filter_device(mpb_ctx *c, const uint8_t *d_q, int64_t n, int64_t row_stride,
                      const int32_t *d_len, int32_t fixed_len, const mpb_filter_params *params,
                      double *d_ee, int32_t *d_ns, uint8_t *d_pass, mpb_filter_counts *counts)
{
    CTXCHK(c);
    int rc = check_params(params);
    if (rc) return rc;
    int32_t max_len = 0;
    if ((rc = check_device_batch(d_q, n, row_stride, d_len, fixed_len, d_ee, d_ns, d_pass, &max_len))) return rc;
    if (counts) { counts->n_reads = n; counts->n_pass = 0; counts->n_fail = 0; counts->n_overflow = 0; }
    if (n == 0) return MPB_OK;
    c->classified.valid = false;                     // the workspace now describes THIS batch
    c->last_path = mpb_path_info{};
    c->classes_whole = true;                         // (unless the narrow pass takes it)
    if ((rc = ensure_workspace(c, 1))) return rc;    // the small block (tables, counters) exists from here on
    if (narrow_eligible(c, n, row_stride, d_len, fixed_len, params)) {
        const MpbDevParams prm = make_dev_params(params, fixed_len, max_len);
        int rows0 = 0, split = 0;
        if ((rc = narrow_choose(c, d_q, n, row_stride, d_len, fixed_len, params, prm, &rows0, &split))) return rc;
        if (rows0) return filter_device_narrow(c, rows0, split, d_q, n, row_stride, d_len, fixed_len, params, prm, d_ee, d_ns, d_pass, counts);
    }
    return filter_device_general(c, d_q, n, row_stride, d_len, fixed_len, max_len, params, d_ee, d_ns, d_pass, counts);
}

int mpb_last_path(mpb_ctx *c, mpb_path_info *out)
{
    CTXCHK(c);
    if (!out) return fail(MPB_E_INVALID, "NULL output");
    *out = c->last_path;
    return MPB_OK;
}

int mpb_last_algorithmic_cells(mpb_ctx *c, int64_t *cells)
{
    CTXCHK(c);
    if (!cells) return fail(MPB_E_INVALID, "NULL output");
    if (!c->ws_small.p) { *cells = 0; return MPB_OK; }
    unsigned long long v = 0;
    int rc = copy_sync(c, &v, c->ws.alg_cells, sizeof(v), hipMemcpyDeviceToHost);
    if (rc) return rc;
    *cells = (int64_t)v;
    return MPB_OK;
}

// ---- classified at source (SURVEY f-4 + VERDICT r2 #6) -------------------------------------------------------------
// A batch that is PRODUCED on the device -- raw FASTQ text decoded into the packed matrix -- is classified by the kernel
// that produces it: the decode pass already holds every byte in registers, so it also sums the prediction statistics,
// counts the ambiguous bases and fills the class histograms.  mpb_filter_device_classified then starts at the scan;
// the packed matrix is read once (by the DP), not twice.

int mpb_decode_classify_device(mpb_ctx *c, const uint8_t *d_seq, const uint8_t *d_qual, int64_t n, int64_t row_stride,
                               const int32_t *d_len, int32_t fixed_len, int32_t fastq_offset,
                               const mpb_filter_params *params, uint8_t *d_q_out, double *d_ee, int32_t *d_ns,
                               uint8_t *d_pass, int32_t *d_err)
{
    CTXCHK(c);
    int rc = check_params(params);
    if (rc) return rc;
    int32_t max_len = 0;
    if ((rc = check_device_batch(d_q_out, n, row_stride, d_len, fixed_len, d_ee, d_ns, d_pass, &max_len))) return rc;
    if ((((uintptr_t)d_seq | (uintptr_t)d_qual) & 15) != 0) return fail(MPB_E_INVALID, "matrices must be 16-byte aligned");
    if (n > 0 && (!d_seq || !d_qual)) return fail(MPB_E_INVALID, "NULL device buffer");
    // the fused pass parks a tile of WHOLE rows in LDS (k_classify_linear: 1,280 chunks): a row of more than 16384 bytes does not
    // fit one -- such text goes through mpb_decode_ascii_device + mpb_filter_device, which take rows of up to 65536 bytes
    if (row_stride > MPB_SMALL_MAX_STRIDE)
        return fail(MPB_E_INVALID, "row_stride %lld: the classify-at-source pass takes rows of up to %d bytes (decode with "
                    "mpb_decode_ascii_device, then mpb_filter_device)", (long long)row_stride, MPB_SMALL_MAX_STRIDE);
    c->classified.valid = false;
    if (n == 0) return MPB_OK;
    if ((rc = prepare_batch(c, n, max_len))) return rc;
    const MpbDevParams prm = make_dev_params(params, fixed_len, max_len);
    { Span t(c, MPB_K_PREPASS);
      mpb_launch_decode_classify(d_seq, d_qual, fastq_offset, d_q_out, d_err, n, row_stride, d_len, prm, c->ws, d_ns, d_ee, d_pass, c->stream); }
    HIPCHK(hipGetLastError());
    c->classified = {true, d_q_out, n, row_stride, d_len, fixed_len, *params, d_ee, d_ns, d_pass};
    return MPB_OK;
}

int mpb_filter_device_classified(mpb_ctx *c, const uint8_t *d_q, int64_t n, int64_t row_stride,
                                 const int32_t *d_len, int32_t fixed_len, const mpb_filter_params *params,
                                 double *d_ee, int32_t *d_ns, uint8_t *d_pass, mpb_filter_counts *counts)
{
    CTXCHK(c);
    int rc = check_params(params);
    if (rc) return rc;
    int32_t max_len = 0;
    if ((rc = check_device_batch(d_q, n, row_stride, d_len, fixed_len, d_ee, d_ns, d_pass, &max_len))) return rc;
    if (counts) { counts->n_reads = n; counts->n_pass = 0; counts->n_fail = 0; counts->n_overflow = 0; }
    if (n == 0) return MPB_OK;
    const auto &k = c->classified;
    const bool same_params = k.valid && memcmp(&k.params.alpha, &params->alpha, sizeof(double)) == 0 &&
                             memcmp(&k.params.uncert, &params->uncert, sizeof(double)) == 0 &&
                             memcmp(&k.params.maxerrors, &params->maxerrors, sizeof(double)) == 0 &&
                             k.params.ambig_mode == params->ambig_mode && k.params.flags == params->flags;
    if (!same_params || k.q != d_q || k.n != n || k.stride != row_stride || k.len != d_len || k.fixed_len != fixed_len ||
        k.ee != d_ee || k.ns != d_ns || k.pass != d_pass)
        return fail(MPB_E_INVALID, "mpb_filter_device_classified: the last call on this context that classified a batch "
                                   "(mpb_decode_classify_device) did not produce THIS batch with THESE parameters and result arrays");
    c->classified.valid = false;                     // consumed: the DP passes overwrite parts of the workspace
    c->classes_whole = true;
    const MpbDevParams prm = make_dev_params(params, fixed_len, max_len);
    return filter_device_tail(c, d_q, n, row_stride, d_len, prm, d_ee, d_ns, d_pass, counts);
}

int mpb_encode_ascii_device(mpb_ctx *c, const uint8_t *d_q, int64_t n, int64_t row_stride, int32_t fastq_offset,
                            uint8_t *d_seq_out, uint8_t *d_qual_out)
{
    CTXCHK(c);
    if (n < 0 || row_stride <= 0 || row_stride % 16 != 0) return fail(MPB_E_INVALID, "bad matrix shape");
    if ((((uintptr_t)d_q | (uintptr_t)d_seq_out | (uintptr_t)d_qual_out) & 15) != 0) return fail(MPB_E_INVALID, "matrices must be 16-byte aligned");
    if (n == 0) return MPB_OK;
    if (!d_q || !d_seq_out || !d_qual_out) return fail(MPB_E_INVALID, "NULL device buffer");
    if (n * (row_stride / 16) / 256 > 0x7fffffffll) return fail(MPB_E_INVALID, "too large for one launch; split it");
    mpb_launch_encode(d_q, n, row_stride, fastq_offset, d_seq_out, d_qual_out, c->stream);
    HIPCHK(hipGetLastError());
    return MPB_OK;
}

int mpb_last_class_histogram(mpb_ctx *c, int32_t *caps, int64_t *cnts, int32_t max_classes)
{
    CTXCHK(c);
    if (!caps || !cnts || max_classes < 0) return fail(MPB_E_INVALID, "bad arguments");
    if (!c->classes_whole)                  // (the workspace then describes the handed-back sub-batch, or an earlier batch: ADVICE r5)
        return fail(MPB_E_INVALID, "the last filter call took the narrow pass (%d rows): there is no class histogram of its batch; "
                                   "call with MPB_FLAG_NO_NARROW to get one", c->last_path.narrow_rows);
    if (!c->ws.tables) return 0;
    static const MpbClass classes[MPB_NCLS] = MPB_CLASS_TABLE;
    MpbTables h;
    int rc = copy_sync(c, &h, c->ws.tables, sizeof(h), hipMemcpyDeviceToHost);
    if (rc) return rc;
    int k = 0;
    for (; k < MPB_NCLS && k < max_classes; k++) { caps[k] = classes[k].cap; cnts[k] = h.count[k]; }
    return k;
}

int mpb_last_read_budgets(mpb_ctx *c, int32_t *caps_out, int64_t n)
{
    CTXCHK(c);
    if (!caps_out || n < 0) return fail(MPB_E_INVALID, "bad arguments");
    if (!c->classes_whole)
        return fail(MPB_E_INVALID, "the last filter call took the narrow pass (%d rows): there are no per-read row budgets of its "
                                   "batch; call with MPB_FLAG_NO_NARROW to get them", c->last_path.narrow_rows);
    if (n > c->ws_cap || !c->ws.cls) return fail(MPB_E_INVALID, "no filter call of at least %lld reads precedes", (long long)n);
    static const MpbClass classes[MPB_NCLS] = MPB_CLASS_TABLE;
    std::vector<uint8_t> cls((size_t)n);
    int rc = copy_sync(c, cls.data(), c->ws.cls, (size_t)n, hipMemcpyDeviceToHost);
    if (rc) return rc;
    for (int64_t i = 0; i < n; i++) {
        const int k = cls[(size_t)i] & 0x7f;
        caps_out[i] = k < MPB_NCLS ? classes[k].cap : 0;
    }
    return MPB_OK;
}

int mpb_decode_ascii_device(mpb_ctx *c, const uint8_t *d_seq, const uint8_t *d_qual, int64_t n, int64_t row_stride,
                            const int32_t *d_len, int32_t fixed_len, int32_t fastq_offset, uint8_t *d_out, int32_t *d_err)
{
    CTXCHK(c);
    if (n < 0 || row_stride <= 0 || row_stride % 16 != 0) return fail(MPB_E_INVALID, "bad matrix shape");
    if ((((uintptr_t)d_seq | (uintptr_t)d_qual | (uintptr_t)d_out) & 15) != 0) return fail(MPB_E_INVALID, "matrices must be 16-byte aligned");
    if (!d_len && (fixed_len < 0 || fixed_len > row_stride)) return fail(MPB_E_INVALID, "fixed_len does not fit row_stride");
    if (n == 0) return MPB_OK;
    if (!d_seq || !d_qual || !d_out) return fail(MPB_E_INVALID, "NULL device buffer");
    if (n * (row_stride / 16) / 256 > 0x7fffffffll) return fail(MPB_E_INVALID, "too large for one launch; split it");
    mpb_launch_decode(d_seq, d_qual, n, row_stride, d_len, fixed_len, fastq_offset, d_out, d_err, c->stream);
    HIPCHK(hipGetLastError());
    return MPB_OK;
}

int mpb_synth_fill_device(mpb_ctx *c, uint8_t *d_q, int64_t n, int64_t row_stride, int32_t fixed_len,
                          int32_t min_len, int32_t max_len, int32_t *d_len, uint64_t seed, int64_t first_read)
{
    return mpb_synth_fill_device_profile(c, d_q, n, row_stride, fixed_len, min_len, max_len, d_len, seed, first_read, 0);
}

int mpb_synth_fill_device_profile(mpb_ctx *c, uint8_t *d_q, int64_t n, int64_t row_stride, int32_t fixed_len,
                                  int32_t min_len, int32_t max_len, int32_t *d_len, uint64_t seed, int64_t first_read,
                                  int32_t profile)
{
    CTXCHK(c);
    if (profile != 0 && profile != 1) return fail(MPB_E_INVALID, "unknown synthetic profile %d", profile);
    if (n < 0 || row_stride <= 0 || row_stride % 16 != 0) return fail(MPB_E_INVALID, "bad matrix shape");
    if (fixed_len > 0) { if (fixed_len > row_stride) return fail(MPB_E_INVALID, "fixed_len exceeds row_stride"); }
    else if (min_len < 1 || max_len < min_len || max_len > row_stride || !d_len)
        return fail(MPB_E_INVALID, "ragged fill needs 1 <= min_len <= max_len <= row_stride and d_len");
    if (n == 0) return MPB_OK;
    if (n * (row_stride / 16) / 256 > 0x7fffffffll) return fail(MPB_E_INVALID, "fill too large for one launch; split it");
    mpb_launch_synth(d_q, n, row_stride, fixed_len, min_len, max_len, d_len, seed, first_read, c->stream, profile);
    HIPCHK(hipGetLastError());
    return MPB_OK;
}
