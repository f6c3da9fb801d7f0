// mpb_hostonly.cpp -- the part of the C ABI of libmoira_pb.so (include/moira_pb.h) that needs no GPU: the error state, the table
// arithmetic (moira/bernoullimodule.c:202,140-145), the packers (moira/bernoullimodule.c:92-108,196), argument checks with the
// reference's error behaviour (moira/bernoullimodule.c:79-90), the cost model that picks the narrow pass, the host tail of the
// Poisson approximation, the NUMA parser.  No HIP header is included here: the unit also builds with a plain C++ compiler, which
// is how tools/asan_api.sh and tools/tsan_poisson.sh run it under the host sanitizers.

#include "mpb_hostonly.h"
#include "contig_posterior.h"            // the two posterior expressions of make_contig (shared with contig.cpp)

#include <cctype>
#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <thread>
#include <unordered_map>
#include <vector>

// (every mpb_* function defined in this file has C linkage: include/moira_pb.h declares it inside extern "C")
#define MPB_VERSION_STR "moira_pb 0.6.0 (gfx950)"

static thread_local char g_err[MPB_ERR_LEN] = "";

int fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

// Threads that copy a pageable input chunk into its pinned staging block: half of the CPUs this process is
// granted (cgroup quota, else the affinity mask), at most 8 -- one memcpy stream does not saturate PCIe 5.
int staging_threads()
{
    int n = (int)std::thread::hardware_concurrency();
    if (n < 1) n = 1;
    if (FILE *f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
        char quota[64]; long long period = 0;
        if (fscanf(f, "%63s %lld", quota, &period) == 2 && strcmp(quota, "max") != 0 && period > 0) {
            const int q = (int)((atoll(quota) + period / 2) / period);
            if (q >= 1 && q < n) n = q;
        }
        fclose(f);
    }
    n = n / 2;
    return n < 1 ? 1 : (n > 8 ? 8 : n);
}

void parallel_copy(void *dst, const void *src, size_t bytes, int threads)
{
    if (threads <= 1 || bytes < (size_t)(8u << 20)) { memcpy(dst, src, bytes); return; }
    const size_t per = ((bytes + (size_t)threads - 1) / (size_t)threads + 4095) & ~(size_t)4095;
    std::vector<std::thread> th;
    size_t done_to = per < bytes ? per : bytes;      // [0, done_to) is this thread's part; helpers take slices above it
    try {
        th.reserve((size_t)threads);
        for (int t = 1; t < threads; t++) {
            const size_t lo = per * (size_t)t;
            if (lo >= bytes) break;
            const size_t len = bytes - lo < per ? bytes - lo : per;
            th.emplace_back([=] { memcpy((char *)dst + lo, (const char *)src + lo, len); });
            done_to = lo + len;
        }
    } catch (...) {
        // no thread to be had (a container's limit): nothing crosses the C ABI as an exception -- what the helpers
        // did not take is copied here
    }
    memcpy(dst, src, bytes < per ? bytes : per);
    for (auto &t : th) t.join();
    if (done_to < bytes) memcpy((char *)dst + done_to, (const char *)src + done_to, bytes - done_to);
}

const char *mpb_version(void) { return MPB_VERSION_STR; }
const char *mpb_last_error(void) { return g_err; }

// {1-p, p'} exactly as the reference evaluates them (ref: moira/bernoullimodule.c:202,140-145):
//   p  = pow(10, q / -10.0)
//   a  = prob_j_errors(p, 0, 1) = pow(1 - p, 1)
//   b  = prob_j_errors(p, 1, 1) = ((1-1+1)/(1.0*1)) * (p/(1-p)) * pow(1 - p, 1)
// evaluated on the host with libm (this unit is built with -ffp-contract=off).  Bytes 0 ('N')
// and 255 ('n') are the identity step of the DP: skipping a base == multiplying by {1, 0}.
// odds != nullptr: also {a, r = p / (1 - p)}, the entry of MPB_FLAG_ODDS' table (a * r is the reference's b before its rounding)
void lut_entry(int q, MpbPair *e, MpbPair *odds)   // any quality the reference's int can hold (p underflows to 0 near Q = 3240)
{
    volatile double p = pow(10, (q / -10.0));
    volatile double a = pow((1 - p), 1);
    volatile double r = p / (1 - p);
    volatile double b1 = ((1 - 1 + 1) / (1.0 * 1)) * r;
    volatile double b = b1 * a;
    e->x = a;
    e->y = b;
    if (odds) { odds->x = a; odds->y = r; }
}

void build_lut(MpbPair *lut, MpbPair *odds)
{
    for (int q = 0; q < 256; q++) {
        if (q == 0 || q == 255) {                       // the identity step, in the odds form too: {1, 0}
            lut[q].x = 1.0; lut[q].y = 0.0;
            if (odds) odds[q] = lut[q];
            continue;
        }
        lut_entry(q, &lut[q], odds ? &odds[q] : nullptr);
    }
}

int mpb_host_lut(double *a_out, double *b_out)
{
    if (!a_out || !b_out) return fail(MPB_E_INVALID, "mpb_host_lut: NULL output");
    MpbPair h[256];
    build_lut(h);
    for (int q = 0; q < 256; q++) { a_out[q] = h[q].x; b_out[q] = h[q].y; }
    return MPB_OK;
}

// ---- packing ---------------------------------------------------------------------------------

static inline uint8_t pack_one(char base, int q)
{
    if (q == 0) q = 1;                       // ref: bernoullimodule.c:104-107
    if (base == 'N') return 0;               // ref: bernoullimodule.c:196 (78)
    if (base == 'n') return 255;             // ref: bernoullimodule.c:196 (110)
    return (uint8_t)q;
}

int mpb_pack_read(const char *seq, const int32_t *quals, int32_t len, uint8_t *row_out, int32_t row_bytes)
{
    if (len < 0 || !row_out || (len > 0 && !quals)) return fail(MPB_E_INVALID, "mpb_pack_read: bad arguments");
    if (len > row_bytes) return fail(MPB_E_INVALID, "read of %d bases does not fit a %d-byte row", len, row_bytes);
    for (int i = 0; i < len; i++) {
        const int q = quals[i];
        if (q < 0) return fail(MPB_E_RANGE, "Qualities must have positive values.");
        if (q > 254) return fail(MPB_E_RANGE, "quality %d at base %d exceeds the encodable maximum 254", q, i);
        row_out[i] = pack_one(seq ? seq[i] : 'A', q);
    }
    memset(row_out + len, 0, (size_t)(row_bytes - len));
    return MPB_OK;
}

int mpb_pack_read_ascii(const char *seq, const char *qual_ascii, int32_t len, int32_t offset,
                        uint8_t *row_out, int32_t row_bytes)
{
    if (len < 0 || !row_out || (len > 0 && !qual_ascii)) return fail(MPB_E_INVALID, "mpb_pack_read_ascii: bad arguments");
    if (len > row_bytes) return fail(MPB_E_INVALID, "read of %d bases does not fit a %d-byte row", len, row_bytes);
    for (int i = 0; i < len; i++) {
        const int q = (int)(unsigned char)qual_ascii[i] - offset;     // ref: moira.py:1177
        if (q < 0) return fail(MPB_E_RANGE, "Qualities must have positive values.");
        if (q > 254) return fail(MPB_E_RANGE, "quality %d at base %d exceeds the encodable maximum 254", q, i);
        row_out[i] = pack_one(seq ? seq[i] : 'A', q);
    }
    memset(row_out + len, 0, (size_t)(row_bytes - len));
    return MPB_OK;
}

int mpb_pack_batch_ascii(const char *seq_cat, const char *qual_cat, const int64_t *off, int64_t n,
                         int32_t fastq_offset, int32_t max_len, int64_t row_stride, uint8_t *out, int32_t *lens_out)
{
    if (n < 0 || row_stride <= 0 || (n > 0 && (!qual_cat || !off || !out))) return fail(MPB_E_INVALID, "mpb_pack_batch_ascii: bad arguments");
    for (int64_t i = 0; i < n; i++) {
        int64_t len = off[i + 1] - off[i];
        if (max_len > 0 && len > max_len) len = max_len;
        if (len < 0 || len > row_stride) return fail(MPB_E_INVALID, "read %lld of %lld bases does not fit a %lld-byte row", (long long)i, (long long)len, (long long)row_stride);
        const char *sq = seq_cat ? seq_cat + off[i] : nullptr;
        const unsigned char *ql = (const unsigned char *)qual_cat + off[i];
        uint8_t *row = out + i * row_stride;
        for (int64_t k = 0; k < len; k++) {
            const int q = (int)ql[k] - fastq_offset;
            if (q < 0) return fail(MPB_E_RANGE, "Qualities must have positive values.");
            if (q > 254) return fail(MPB_E_RANGE, "quality %d exceeds the encodable maximum 254", q);
            row[k] = pack_one(sq ? sq[k] : 'A', q);
        }
        memset(row + len, 0, (size_t)(row_stride - len));
        if (lens_out) lens_out[i] = (int32_t)len;
    }
    return MPB_OK;
}

// The row descriptors k_pack_text walks, from a record index (include/moira_io.h's six columns, restated in moira_pb.h).  This is
// the only place the offsets of a text are trusted from: every one is checked against the text here, before anything is uploaded.
int mpb_text_rows(const int64_t *idx, int64_t n_records, const int64_t *sel, int64_t n, int64_t text_bytes, int32_t max_len,
                  int64_t row_stride, mpb_text_row *rows_out, int64_t *longest_out, int64_t *bad_record)
{
    if (bad_record) *bad_record = -1;
    if (longest_out) *longest_out = 0;
    if (n < 0 || n_records < 0 || text_bytes < 0 || row_stride < 0 || (n > 0 && !idx) || (n_records > 0 && !idx))
        return fail(MPB_E_INVALID, "mpb_text_rows: bad arguments");
    if (row_stride > 0 && n > 0 && !rows_out) return fail(MPB_E_INVALID, "mpb_text_rows: rows_out is NULL");
    if (!sel && n > n_records) return fail(MPB_E_INVALID, "mpb_text_rows: %lld rows asked of an index of %lld records", (long long)n, (long long)n_records);
    int64_t longest = 0;
    for (int64_t k = 0; k < n; k++) {
        auto bad = [&](const char *what, long long v) {
            if (bad_record) *bad_record = k;
            return fail(MPB_E_INVALID, "record at position %lld: %s (%lld)", (long long)k, what, v);
        };
        const int64_t r = sel ? sel[k] : k;
        if (r < 0 || r >= n_records) return bad("sel entry outside the index", (long long)r);
        const int64_t *row = idx + r * MPB_IDX_COLS;
        const int64_t so = row[MPB_IDX_SEQ_OFF], qo = row[MPB_IDX_QUAL_OFF];
        int64_t len = row[MPB_IDX_QUAL_LEN];
        if (so < 0) return bad("negative sequence offset", (long long)so);
        if (qo < 0) return bad("negative quality offset", (long long)qo);
        if (len < 0) return bad("negative length", (long long)len);
        if (max_len > 0 && len > max_len) len = max_len;                 // mio_pack's rule
        if (len > MPB_MAX_LEN) return bad("reads longer than 65535 bases are not supported; length", (long long)len);
        if (len > text_bytes || so > text_bytes - len) return bad("the sequence line ends past the text; offset", (long long)so);
        if (qo > text_bytes - len) return bad("the quality line ends past the text; offset", (long long)qo);
        if (row_stride > 0 && len > row_stride) return bad("the read does not fit the row; length", (long long)len);
        if (len > longest) longest = len;
        if (row_stride > 0) { rows_out[k].seq_off = so; rows_out[k].qual_off = qo; rows_out[k].len = (int32_t)len; rows_out[k].pad = 0; }
    }
    if (longest_out) *longest_out = longest;
    return MPB_OK;
}

// The pair descriptors k_contig walks, from the two record indexes (columns: header offset 0, header length 1, sequence offset 2,
// sequence length 3, quality offset 4, quality length 5).  As mpb_text_rows: validation, never clamping; the kernel rechecks.
int mpb_pair_rows(const int64_t *fidx, const int64_t *ridx, int64_t n, int64_t ftext_bytes, int64_t rtext_bytes, int64_t rec_cap,
                  mpb_pair_row *rows_out, int64_t *bad_record)
{
    if (bad_record) *bad_record = -1;
    if (n < 0 || ftext_bytes < 0 || rtext_bytes < 0 || rec_cap <= 0 || (n > 0 && (!fidx || !ridx || !rows_out)))
        return fail(MPB_E_INVALID, "mpb_pair_rows: bad arguments");
    for (int64_t i = 0; i < n; i++) {
        auto bad = [&](const char *what, long long v) {
            if (bad_record) *bad_record = i;
            return fail(MPB_E_INVALID, "pair %lld: %s (%lld)", (long long)i, what, v);
        };
        const int64_t *f = fidx + i * MPB_IDX_COLS, *r = ridx + i * MPB_IDX_COLS;
        const int64_t ho = f[0], hl = f[1], l1 = f[3], l2 = r[3];
        if (ho < 0 || hl < 0) return bad("negative header offset or length", (long long)(ho < 0 ? ho : hl));
        if (hl > ftext_bytes || ho > ftext_bytes - hl) return bad("the header ends past the text; offset", (long long)ho);
        if (l1 < 0 || l2 < 0) return bad("negative length", (long long)(l1 < 0 ? l1 : l2));
        if (l1 > 0x7fffffffll || l2 > 0x7fffffffll || hl > 0x7fffffffll) return bad("length above 2^31 - 1", (long long)(l1 > l2 ? l1 : l2));
        if (f[MPB_IDX_QUAL_LEN] != l1) return bad("forward sequence and quality lines differ in length; quality length", (long long)f[MPB_IDX_QUAL_LEN]);
        if (r[MPB_IDX_QUAL_LEN] != l2) return bad("reverse sequence and quality lines differ in length; quality length", (long long)r[MPB_IDX_QUAL_LEN]);
        const int64_t fs = f[MPB_IDX_SEQ_OFF], fq = f[MPB_IDX_QUAL_OFF], rs = r[MPB_IDX_SEQ_OFF], rq = r[MPB_IDX_QUAL_OFF];
        if (fs < 0 || fq < 0 || rs < 0 || rq < 0) return bad("negative offset", (long long)(fs < 0 ? fs : fq < 0 ? fq : rs < 0 ? rs : rq));
        if (l1 > ftext_bytes || fs > ftext_bytes - l1) return bad("the forward sequence line ends past the text; offset", (long long)fs);
        if (fq > ftext_bytes - l1) return bad("the forward quality line ends past the text; offset", (long long)fq);
        if (l2 > rtext_bytes || rs > rtext_bytes - l2) return bad("the reverse sequence line ends past the text; offset", (long long)rs);
        if (rq > rtext_bytes - l2) return bad("the reverse quality line ends past the text; offset", (long long)rq);
        if (hl + 2 * (l1 + l2) > rec_cap) return bad("the contig does not fit rec_cap; bytes needed", (long long)(hl + 2 * (l1 + l2)));
        mpb_pair_row &o = rows_out[i];
        o.fseq_off = fs; o.fqual_off = fq; o.fhdr_off = ho; o.rseq_off = rs; o.rqual_off = rq;
        o.l1 = (int32_t)l1; o.l2 = (int32_t)l2; o.hdr_len = (int32_t)hl; o.pad = 0;
    }
    return MPB_OK;
}

int mpb_contig_posterior_tables(int32_t *match_out, int32_t *mismatch_out)
{
    if (!match_out || !mismatch_out) return fail(MPB_E_INVALID, "mpb_contig_posterior_tables: NULL table");
    // prob2qual = (int)floor(-10 log10 p), kept out of the cast where it is no finite integer
    auto q_of = [](double p) {
        const double v = floor(-10 * log10(p));
        return (v > -2e9 && v < 2e9) ? (int32_t)v : INT32_MIN;
    };
    for (int f = 0; f < 256; f++)
        for (int r = 0; r < 256; r++) {
            match_out[f * 256 + r] = q_of(posterior_match_p(f, r));
            mismatch_out[f * 256 + r] = f == r ? 2 : q_of(posterior_mismatch_p(f, r));
        }
    return MPB_OK;
}

// Phi^-1 (Acklam's rational approximation, |rel err| < 1.2e-9): only steers the row-budget
// prediction, never a result.
double inv_norm_cdf(double p)
{
    static const double a[] = {-3.969683028665376e+01, 2.209460984245205e+02, -2.759285104469687e+02,
                               1.383577518672690e+02, -3.066479806614716e+01, 2.506628277459239e+00};
    static const double b[] = {-5.447609879822406e+01, 1.615858368580409e+02, -1.556989798598866e+02,
                               6.680131188771972e+01, -1.328068155288572e+01};
    static const double cc[] = {-7.784894002430293e-03, -3.223964580411365e-01, -2.400758277161838e+00,
                                -2.549732539343734e+00, 4.374664141464968e+00, 2.938163982698783e+00};
    static const double d[] = {7.784695709041462e-03, 3.224671290700398e-01, 2.445134137142996e+00,
                               3.754408661907416e+00};
    const double pl = 0.02425;
    if (p < pl) {
        double q = sqrt(-2 * log(p));
        return (((((cc[0] * q + cc[1]) * q + cc[2]) * q + cc[3]) * q + cc[4]) * q + cc[5]) /
               ((((d[0] * q + d[1]) * q + d[2]) * q + d[3]) * q + 1);
    }
    if (p > 1 - pl) {
        double q = sqrt(-2 * log(1 - p));
        return -(((((cc[0] * q + cc[1]) * q + cc[2]) * q + cc[3]) * q + cc[4]) * q + cc[5]) /
               ((((d[0] * q + d[1]) * q + d[2]) * q + d[3]) * q + 1);
    }
    double q = p - 0.5, r = q * q;
    return (((((a[0] * r + a[1]) * r + a[2]) * r + a[3]) * r + a[4]) * r + a[5]) * q /
           (((((b[0] * r + b[1]) * r + b[2]) * r + b[3]) * r + b[4]) * r + 1);
}

int check_params(const mpb_filter_params *p)
{
    if (!p) return fail(MPB_E_INVALID, "params is NULL");
    if (!(p->alpha > 0 && p->alpha < 1))                       // ref: bernoullimodule.c:79-83
        return fail(MPB_E_INVALID, "Alpha must be between 0 and 1");
    if (p->ambig_mode < 0 || p->ambig_mode > 2) return fail(MPB_E_INVALID, "unknown ambig_mode %d", p->ambig_mode);
    if ((p->flags & MPB_FLAG_FAST_FMA) && p->alpha < 1e-5)      // the fma error grows like 1/alpha (include/moira_pb.h)
        return fail(MPB_E_INVALID, "MPB_FLAG_FAST_FMA needs alpha >= 1e-5 (its error bound does not hold below)");
    if ((p->flags & MPB_FLAG_ODDS) && (p->flags & MPB_FLAG_FAST_FMA))
        return fail(MPB_E_INVALID, "MPB_FLAG_ODDS and MPB_FLAG_FAST_FMA are two arithmetics for the same pass: set one");
    if ((p->flags & MPB_FLAG_ODDS_NARROW) && !(p->flags & MPB_FLAG_ODDS))
        return fail(MPB_E_INVALID, "MPB_FLAG_ODDS_NARROW needs MPB_FLAG_ODDS");
    if ((p->flags & MPB_FLAG_ODDS) && p->alpha < 1e-5)          // the same 1/alpha growth (include/moira_pb.h)
        return fail(MPB_E_INVALID, "MPB_FLAG_ODDS needs alpha >= 1e-5 (its error bound does not hold below)");
    const bool has_me = p->maxerrors == p->maxerrors;
    if (has_me && !(p->maxerrors > 0)) return fail(MPB_E_INVALID, "maxerrors must be > 0");           // moira.py:732
    if (!has_me && !(p->uncert > 0 && p->uncert <= 1)) return fail(MPB_E_INVALID, "uncert must be in (0,1]");  // moira.py:728
    return MPB_OK;
}

int check_text_bytes(int64_t text_bytes)
{
    if (text_bytes <= k_text_max_bytes) return MPB_OK;
    return fail(MPB_E_INVALID, "text of %lld bytes: one call takes at most %lld bytes (1 GiB) of text; split the chunk",
                (long long)text_bytes, (long long)k_text_max_bytes);
}

int check_fastq_offset(int32_t fastq_offset, const char *who)
{
    if (fastq_offset >= 0 && fastq_offset <= 255) return MPB_OK;
    return fail(MPB_E_INVALID, "%s%sfastq_offset %d: the device pack takes offsets 0..255 (beyond them no character is a quality)",
                who ? who : "", who ? ": " : "", fastq_offset);
}

int64_t env_int64(const char *name, int64_t lo, int64_t hi, int64_t fallback)
{
    const char *e = getenv(name);
    const long long v = e ? atoll(e) : 0;
    return e && v >= lo && v <= hi ? (int64_t)v : fallback;
}

// The choice, from the sample's histogram of rows.  Costs per read in units of 0.083 ms per 10 M reads of 300 bases, fitted to
// measured steps (profiles/r05_narrow_rate.txt; round 6: profiles/r06_narrow_mix.txt, r06_ragged_mix.txt): the narrow pass 4 + 3 R for
// every read whatever it needs; the sorted pipeline 9 (classification + sort: its second read of the matrix) + 3.9 per row of the
// read's class (its predictor gives the few-row reads one row more than they need); a read the narrow pass hands back pays the sorted
// pipeline's cost x 1.05 + 1 -- since round 6 it runs through that pipeline where it lies (round 5 gathered it into a dense sub-batch:
// x 1.3 + 3), so the pass wins up to about 40 % handed back (round 5: 20 %).  The pass must finish at least 55 % of the sample and
// promise at least 5 %.
//
// MPB_FLAG_ODDS_NARROW has constants of its own, in the same unit, fitted to the first of two runs of tools/odds_narrow_rate.py
// (profiles/odds_narrow_rate_fit.txt; 10 M x 300, alternating options, 3 rounds x 20 steps; the second run, on another box 2-3 %
// slower throughout, is profiles/odds_narrow_rate.json):
//   the pass       forced R = 2 / 3 / 4 on the clean batch: 0.705 / 0.730 / 0.821 ms = 8.5 / 8.8 / 9.9 units; least squares 7.0 + 0.7 R
//                  (a row is one operation here, and the pass is no longer bound by its arithmetic: ODDS_MODE.md)
//   sorted + odds  the clean batch (every read in the class of cap 3): 1.638 ms = 19.7; BASELINE's reads: 28.8 per read from the slope
//                  of the odds-alone step over the 5 / 20 / 40 % mixes (1.670 / 1.782 / 1.940 ms), config 2 as a whole 2.34 ms = 28.2
//                  (ODDS_MODE.md); their mean cap is 9.6 by the exact constants (3.84 ms = 9 + 3.9 cap).  Two points: 15.7 + 1.34 cap
//                  (k_dp_odds moves more than it computes on few-row classes: a larger intercept, a third of the slope)
//   handed back    forced R = 2 on the mixes: the step less the pure pass is 0.194 / 0.553 / 1.032 ms for 0.50 / 2.00 / 4.00 M reads =
//                  0.074 ms per call (0.9 units per read of the batch: the second pipeline's launches and its synchronisation) +
//                  28.8 per read: the sorted cost itself, no factor
// Flat Q30 and Q25-32 batches were not measured in this mode.  Checked on the second run: the model's R is the fastest forced option
// on the clean batch, on every mix (R = 2 / 2 / 3 / 4 at 0 / 5 / 20 / 40 %) and on the ragged clean batch (R = 3), within 1 %.
struct NarCostModel { double u0, u1, s0, s1, back_mul, back_add, back_call; };   // narrow u0 + u1 R; sorted s0 + s1 cap; a read handed
                                                                                 // back: sorted x back_mul + back_add; any: back_call per read of the batch
static const NarCostModel nar_cost_exact = {4.0, 3.0, 9.0, 3.9, 1.05, 1.0, 0.0};
static const NarCostModel nar_cost_odds = {7.0, 0.7, 15.7, 1.34, 1.0, 0.0, 0.9};
int narrow_rows_from_sample(const int32_t *hist, int n_sample, bool odds)
{
    if (n_sample <= 0) return 0;
    const NarCostModel &m = odds ? nar_cost_odds : nar_cost_exact;
    auto sorted_cost = [&m](int r) {
        const int cap = r == MPB_NAR_BUCKETS - 1 ? 30 : r <= 4 ? (r < 1 ? 2 : r + 1) : r;
        return m.s0 + m.s1 * cap;
    };
    const double lower_n_cost = sorted_cost(6);              // a read with a lower-case 'n' (handed back by the pass): a middling class
    double general = hist[0] * lower_n_cost;
    for (int r = 1; r < MPB_NAR_BUCKETS; r++) general += hist[r] * sorted_cost(r);
    int best = 0;
    double best_cost = 0.95 * general;
    for (int R = MPB_NAR_MIN_ROWS; R <= MPB_NAR_MAX_ROWS; R++) {
        int64_t done = 0;
        for (int r = 1; r <= R; r++) done += hist[r];
        if ((double)done < 0.55 * n_sample) continue;
        double cost = (double)n_sample * (m.u0 + m.u1 * R) + hist[0] * (m.back_mul * lower_n_cost + m.back_add);
        for (int r = R + 1; r < MPB_NAR_BUCKETS; r++) cost += hist[r] * (m.back_mul * sorted_cost(r) + m.back_add);
        if ((int64_t)n_sample > done) cost += (double)n_sample * m.back_call;
        if (cost < best_cost) { best = R; best_cost = cost; }
    }
    return best;
}

// qualities per chunk of the host pipeline: large enough that a chunk's launch sequence (~0.2 ms fixed) is
// noise beside its 2 ms of PCIe time; the four slots then hold 4 x (128 MiB of qualities + 5.5 MiB of results) of device
// memory, the same again of pinned staging when the input is pageable, and 4 x 5.5 MiB of pinned results
#define MPB_HOST_CHUNK_BYTES (128ll << 20)

// reads per chunk of a batch of n reads
int64_t pipeline_chunk_reads(int64_t n, int64_t row_stride)
{
    // chunk: at most MPB_HOST_CHUNK_BYTES of qualities, and at least four chunks per batch where the batch
    // is large enough for a chunk to be worth a launch sequence (overlap needs more than one chunk)
    int64_t chunk = (int64_t)MPB_HOST_CHUNK_BYTES / row_stride;
    if (chunk > (n + 3) / 4) chunk = (n + 3) / 4;
    {   // ... but not below 16384 reads (a launch sequence's worth), nor -- rows of up to 64 KiB -- above 256 MiB for that floor
        int64_t floor_reads = (256ll << 20) / row_stride;
        if (floor_reads > 16384) floor_reads = 16384;
        if (floor_reads < 256) floor_reads = 256;
        if (chunk < floor_reads) chunk = floor_reads;
    }
    if (chunk > n) chunk = n;
    return chunk;
}

// One read of the per-read entries -> a packed row.  A score the byte codes cannot express borrows a code the read does
// not use, from 254 down (the row predictor reads codes as scores, and up there every code means "practically never
// wrong"), and h -- a copy of the context's table -- gets {1-p, p'} of the real score under that code (*priv = true):
// the reference takes any int (moira/bernoullimodule.c:92-108, moira/moira.py:1637-1679) and one read holds few
// distinct values.  poisson: the Python function's rules -- 'n' is a base like any other (moira.py:1660), Q0 is p = 1
// (no clamp inside the function; it too gets a private code), and the second table component is p itself.
int pack_one_read(const char *contig, const int32_t *quals, int32_t len, bool poisson, uint8_t *row, int32_t row_bytes,
                  MpbPair *h, bool *priv)
{
    *priv = false;
    auto direct = [&](int32_t q) { return poisson ? (q >= 1 && q <= 254) : q <= 254; };
    bool used[256] = {};
    for (int32_t i = 0; i < len; i++) {
        const int32_t q = quals[i];
        if (q < 0) return fail(MPB_E_RANGE, "Qualities must have positive values.");
        if (direct(q)) used[q == 0 ? 1 : q] = true; else *priv = true;
    }
    if (*priv) build_lut(h);
    std::unordered_map<int32_t, int> code_of;
    int next = 254;
    for (int32_t i = 0; i < len; i++) {
        const int32_t q = quals[i];
        char base = contig ? contig[i] : 'A';
        if (poisson && base == 'n') base = 'A';
        if (direct(q)) { row[i] = pack_one(base, q); continue; }
        auto it = code_of.find(q);
        if (it == code_of.end()) {
            while (next >= 1 && used[next]) next--;
            if (next < 1) return fail(MPB_E_RANGE, "more than 254 distinct quality values in one read, some outside 1..254");
            used[next] = true;
            lut_entry(q, &h[next]);
            if (poisson) { volatile double p = pow(10, (q / -10.0)); h[next].y = p; }     // (1 - p is 0 at Q0: p' is not p there)
            it = code_of.emplace(q, next).first;
        }
        row[i] = pack_one(base, it->second);
    }
    memset(row + len, 0, (size_t)(row_bytes - len));
    return MPB_OK;
}

// ---- batches whose reads carry scores above 254 (missing 3: the reference takes any int) ----------------
// The byte matrix has 254 score codes.  A batch rarely uses them all, so -- exactly as the per-read entry does for one read --
// the packer gives every distinct out-of-range score of the BATCH a code the batch does not use (from 254 down: the row
// predictor reads codes as scores, and up there every code means "practically never wrong") and reports what each code
// stands for; mpb_filter_host_coded runs the ordinary pipeline on a private copy of the table built from that list.

int mpb_pack_batch_coded(const char *seq_cat, const int32_t *qual_cat, const int64_t *off, int64_t n, int32_t max_len,
                         int64_t row_stride, uint8_t *q_out, int32_t *len_out, int32_t *code_scores)
{
    if (!qual_cat || !off || !q_out || !len_out || !code_scores || n < 0) return fail(MPB_E_INVALID, "bad arguments");
    if (row_stride <= 0 || row_stride % 16 != 0) return fail(MPB_E_INVALID, "row_stride must be a positive multiple of 16");
    bool used[256] = {};
    std::unordered_map<int32_t, int> code_of;
    std::vector<int32_t> big;                         // distinct out-of-range scores in order of first appearance
    for (int64_t i = 0; i < n; i++) {
        int64_t L = off[i + 1] - off[i];
        if (L < 0) return fail(MPB_E_INVALID, "offsets must not decrease");
        if (max_len > 0 && L > max_len) L = max_len;
        if (L > row_stride) return fail(MPB_E_INVALID, "read %lld (%lld bases) does not fit row_stride %lld", (long long)i, (long long)L, (long long)row_stride);
        if (L > MPB_MAX_LEN) return fail(MPB_E_INVALID, "read %lld has %lld bases: reads longer than %d bases are not supported", (long long)i, (long long)L, MPB_MAX_LEN);
        for (int64_t k = 0; k < L; k++) {
            const int32_t q = qual_cat[off[i] + k];
            if (q < 0) return fail(MPB_E_RANGE, "Qualities must have positive values.");
            if (q <= 254) used[q == 0 ? 1 : q] = true;
            else if (code_of.emplace(q, -1).second) big.push_back(q);
        }
    }
    for (int c = 0; c < 256; c++) code_scores[c] = c;
    int next = 254;
    size_t assigned = 0;
    for (int32_t q : big) {
        while (next >= 1 && used[next]) next--;
        if (next < 1)
            return fail(MPB_E_RANGE, "the batch holds %zu distinct scores above 254 but uses all but %zu of the 254 byte codes: "
                        "split it (or score such reads through mpb_calculate_errors_PB)", big.size(), assigned);
        assigned++;
        used[next] = true;
        code_of[q] = next;
        code_scores[next] = q;
    }
    for (int64_t i = 0; i < n; i++) {
        int64_t L = off[i + 1] - off[i];
        if (max_len > 0 && L > max_len) L = max_len;
        uint8_t *row = q_out + i * row_stride;
        for (int64_t k = 0; k < L; k++) {
            const int32_t q = qual_cat[off[i] + k];
            const char base = seq_cat ? seq_cat[off[i] + k] : 'A';
            row[k] = pack_one(base, q <= 254 ? q : code_of[q]);
        }
        memset(row + L, 0, (size_t)(row_stride - L));
        len_out[i] = (int32_t)L;
    }
    return MPB_OK;
}

// float(math.factorial(j)) for j = 0..170: exact up to 22!, correctly rounded above (built from
// the exact integer with round-half-even on first use).
struct FactorialTable {
    double tab[171];
    FactorialTable()
    {
        // exact big-integer product in base 2^32, then correctly rounded conversion
        std::vector<uint32_t> big(1, 1u);
        tab[0] = 1.0;
        for (int j = 1; j <= 170; j++) {
            uint64_t carry = 0;
            for (size_t k = 0; k < big.size(); k++) {
                uint64_t v = (uint64_t)big[k] * (uint64_t)j + carry;
                big[k] = (uint32_t)v; carry = v >> 32;
            }
            if (carry) big.push_back((uint32_t)carry);
            // top 64+ bits -> double with round-half-even
            int top = (int)big.size() - 1;
            int hb = 31; while (!((big[top] >> hb) & 1u)) hb--;
            const long nbits = (long)top * 32 + hb + 1;
            auto bit = [&](long pos) -> int { return pos < 0 ? 0 : (int)((big[pos / 32] >> (pos % 32)) & 1u); };
            uint64_t mant = 0;
            for (int k = 0; k < 53; k++) mant = (mant << 1) | (uint64_t)bit(nbits - 1 - k);
            if (nbits > 53) {
                const int guard = bit(nbits - 54);
                bool sticky = false;
                for (long pos = nbits - 55; pos >= 0 && !sticky; pos--) sticky = bit(pos) != 0;
                if (guard && (sticky || (mant & 1u))) mant++;
            }
            tab[j] = ldexp((double)mant, nbits > 53 ? (int)(nbits - 53) : 0);
            if (nbits <= 53) tab[j] = (double)mant / ldexp(1.0, (int)(53 - nbits));
        }
    }
};

static const double *factorial_table()
{
    // function-local static object: initialised once, thread-safe (C++11 magic static) -- contexts on different
    // threads may reach the Poisson path for the first time concurrently
    static const FactorialTable t;
    return t.tab;
}

// ref: moira/moira.py:1666-1679 -- one read
static double poisson_tail(double lam, double alpha, const double *fact)
{
    double acc_prev = 0, acc = 0;
    int j = 0;
    const double em = exp(-lam);                                  // the reference re-evaluates it per term: same value
    for (;;) {
        if (j > 170) return NAN;                                  // Python: int too large to convert to float
        const double pw = pow(lam, (double)j);
        if (std::isinf(pw)) return NAN;                           // Python: OverflowError from float pow
        const double prob = (em * pw) / fact[j];
        acc_prev = acc;
        acc = acc_prev + prob;
        if (acc > (1 - alpha)) break;
        j++;
    }
    double r = (j - 1) + ((j - (j - 1)) * ((1 - alpha) - acc_prev) / (acc - acc_prev));
    if (r < 0) r = 0;
    return r;
}

int mpb_poisson_finish_host(const double *lambda, const int32_t *ns, const int32_t *len, int32_t fixed_len,
                            int64_t n, const mpb_filter_params *p, double *ee, uint8_t *pass)
{
    int rc = check_params(p);
    if (rc) return rc;
    if (n < 0 || (n > 0 && (!lambda || !ns || !ee || !pass))) return fail(MPB_E_INVALID, "bad arguments");
    const double *fact = factorial_table();
    auto run = [=](int64_t lo, int64_t hi) {
        for (int64_t i = lo; i < hi; i++) {
            double e = mpb_add_ns(*p, poisson_tail(lambda[i], p->alpha, fact), ns[i]);
            const bool keep = mpb_round_and_keep(*p, e, ns[i] > 0, len ? len[i] : fixed_len);    // (ns counts 'N' only here)
            ee[i] = e;
            pass[i] = keep ? 1 : 0;
        }
    };
    // the scalar tail (one libm pow per CDF term) is what a GPU-fed Poisson run waits for: reads are independent,
    // so large batches are split over the CPUs this process is granted (each read's arithmetic is unchanged)
    const int threads = n >= 16384 ? 2 * staging_threads() : 1;
    if (threads <= 1) { run(0, n); return MPB_OK; }
    std::vector<std::thread> th;
    const int64_t per = (n + threads - 1) / threads;
    int64_t taken = per < n ? per : n;                 // helpers take [per, taken); the rest is done here
    try {
        th.reserve((size_t)threads);
        for (int t = 1; t < threads; t++) {
            const int64_t lo = per * t, hi = lo + per < n ? lo + per : n;
            if (lo >= n) break;
            th.emplace_back(run, lo, hi);
            taken = hi;
        }
    } catch (...) {
        // thread creation failed: never an exception across the C ABI, the remainder runs on this thread
    }
    run(0, per < n ? per : n);
    if (taken < n) run(taken, n);
    for (auto &t : th) t.join();
    return MPB_OK;
}

// The reads of a batch in HOST arrays that k_poisson_tail handed back (pass byte 2, lambda in the ee slot): the host tail on exactly
// those, through mpb_poisson_finish_host on a dense copy (so a batch that is handed back as a whole is split over the CPUs).
int poisson_finish_marked(const mpb_filter_params *p, const int32_t *ns, const int32_t *len, int32_t fixed_len, int64_t n,
                                 double *ee, uint8_t *pass, int64_t *n_marked)
{
    *n_marked = 0;
    const uint8_t *first = (const uint8_t *)memchr(pass, 2, (size_t)n);
    if (!first) return MPB_OK;
    try {
        std::vector<int64_t> idx;
        for (int64_t i = first - pass; i < n; i++) if (pass[i] == 2) idx.push_back(i);
        const size_t m = idx.size();
        std::vector<double> lam(m), e(m);
        std::vector<int32_t> nsv(m), lv(m);
        std::vector<uint8_t> ps(m);
        for (size_t k = 0; k < m; k++) { lam[k] = ee[idx[k]]; nsv[k] = ns[idx[k]]; lv[k] = len ? len[idx[k]] : fixed_len; }
        int rc = mpb_poisson_finish_host(lam.data(), nsv.data(), lv.data(), 0, (int64_t)m, p, e.data(), ps.data());
        if (rc) return rc;
        for (size_t k = 0; k < m; k++) { ee[idx[k]] = e[k]; pass[idx[k]] = ps[k]; }
        *n_marked = (int64_t)m;
    } catch (const std::bad_alloc &) {
        return fail(MPB_E_NOMEM, "out of host memory for the reads handed back to the host tail");
    }
    return MPB_OK;
}

static bool read_small_file(const char *path, char *buf, size_t len)
{
    FILE *f = fopen(path, "r");
    if (!f) return false;
    const size_t k = fread(buf, 1, len - 1, f);
    fclose(f);
    buf[k] = 0;
    return k > 0;
}

// "0-7,16-23,40" -> cpu_set; false on anything else
bool parse_cpulist(const char *s, cpu_set_t *set, int *count)
{
    CPU_ZERO(set);
    int n = 0;
    const char *p = s;
    while (*p && *p != '\n') {
        char *end = nullptr;
        const long a = strtol(p, &end, 10);
        if (end == p || a < 0) return false;
        long b = a;
        p = end;
        if (*p == '-') {
            b = strtol(p + 1, &end, 10);
            if (end == p + 1 || b < a) return false;
            p = end;
        }
        for (long c = a; c <= b; c++)
            if (c < CPU_SETSIZE) { CPU_SET((int)c, set); n++; }
        if (*p == ',') p++;
        else if (*p && *p != '\n') return false;
    }
    if (count) *count = n;
    return n > 0;
}

int mpb_numa_cpulist_for_pci(const char *sysfs_root, const char *pci_bus_id, int32_t *node_out, char *cpulist_out, int32_t cpulist_len)
{
    if (!pci_bus_id || !node_out) return fail(MPB_E_INVALID, "mpb_numa_cpulist_for_pci: NULL argument");
    const char *root = sysfs_root ? sysfs_root : "";
    char path[512], buf[4096], id[64];
    // HIP prints the bus id in upper-case hex ("0000:C1:00.0"); sysfs names are lower-case
    size_t k = 0;
    for (; pci_bus_id[k] && k + 1 < sizeof(id); k++) id[k] = (char)tolower((unsigned char)pci_bus_id[k]);
    id[k] = 0;
    *node_out = -1;
    if (cpulist_out && cpulist_len > 0) cpulist_out[0] = 0;
    snprintf(path, sizeof(path), "%s/sys/bus/pci/devices/%s/numa_node", root, id);
    if (!read_small_file(path, buf, sizeof(buf))) return MPB_OK;          // no such file: no NUMA information
    char *end = nullptr;
    const long node = strtol(buf, &end, 10);
    if (end == buf || node < 0) return MPB_OK;                               // "-1": the platform does not say
    snprintf(path, sizeof(path), "%s/sys/devices/system/node/node%ld/cpulist", root, node);
    if (!read_small_file(path, buf, sizeof(buf))) return MPB_OK;
    cpu_set_t set;
    int cnt = 0;
    if (!parse_cpulist(buf, &set, &cnt)) return fail(MPB_E_INVALID, "cannot parse %s: '%s'", path, buf);
    *node_out = (int32_t)node;
    if (cpulist_out && cpulist_len > 0) {
        snprintf(cpulist_out, (size_t)cpulist_len, "%s", buf);
        for (char *q = cpulist_out; *q; q++) if (*q == '\n') *q = 0;
    }
    return MPB_OK;
}

int mpb_shard_bounds(int64_t n, int32_t world, int32_t rank, int64_t *lo, int64_t *hi)
{
    if (n < 0 || world < 1 || rank < 0 || rank >= world || !lo || !hi) return fail(MPB_E_INVALID, "mpb_shard_bounds: bad arguments");
    const int64_t base = n / world, rem = n % world;
    *lo = rank * base + (rank < rem ? rank : rem);
    *hi = *lo + base + (rank < rem ? 1 : 0);
    return MPB_OK;
}

// ---- .gz output on the device: the host's share (the bound, and the CRC-32 of every member while the kernels run) -----------------
int mpb_bgzf_bound(int64_t text_bytes, int64_t *out_cap)
{
    if (text_bytes < 0 || !out_cap) return fail(MPB_E_INVALID, "mpb_bgzf_bound: bad arguments");
    if (text_bytes > (int64_t)1 << 56) return fail(MPB_E_INVALID, "mpb_bgzf_bound: %lld bytes of text", (long long)text_bytes);
    const int64_t members = (text_bytes + MPB_BGZF_DATA - 1) / MPB_BGZF_DATA;
    *out_cap = text_bytes + 31 * members;                  // every member stored: 18 + 5 + text + 8
    return MPB_OK;
}

namespace {
struct BgzfCrcTables {                                     // RFC 1952 section 8, eight bytes per step
    uint32_t t[8][256];
    BgzfCrcTables()
    {
        for (uint32_t i = 0; i < 256; i++) {
            uint32_t c = i;
            for (int k = 0; k < 8; k++) c = (c & 1) ? 0xedb88320u ^ (c >> 1) : c >> 1;
            t[0][i] = c;
        }
        for (uint32_t i = 0; i < 256; i++)
            for (int k = 1; k < 8; k++) t[k][i] = t[0][t[k - 1][i] & 0xff] ^ (t[k - 1][i] >> 8);
    }
};
const BgzfCrcTables g_bgzf_crc;
}  // namespace

uint32_t bgzf_crc32(const uint8_t *p, size_t n)
{
    uint32_t c = 0xffffffffu;
    while (n >= 8) {
        uint64_t v;
        memcpy(&v, p, 8);
        v ^= c;
        c = g_bgzf_crc.t[7][v & 0xff] ^ g_bgzf_crc.t[6][(v >> 8) & 0xff] ^ g_bgzf_crc.t[5][(v >> 16) & 0xff] ^
            g_bgzf_crc.t[4][(v >> 24) & 0xff] ^ g_bgzf_crc.t[3][(v >> 32) & 0xff] ^ g_bgzf_crc.t[2][(v >> 40) & 0xff] ^
            g_bgzf_crc.t[1][(v >> 48) & 0xff] ^ g_bgzf_crc.t[0][v >> 56];
        p += 8; n -= 8;
    }
    while (n--) c = g_bgzf_crc.t[0][(c ^ *p++) & 0xff] ^ (c >> 8);
    return ~c;
}

void bgzf_member_crcs(const uint8_t *text, int64_t text_bytes, int64_t n_members, uint32_t *crc_out)
{
    auto run = [=](int64_t lo, int64_t hi) {
        for (int64_t m = lo; m < hi; m++) {
            const int64_t off = m * (int64_t)MPB_BGZF_DATA;
            const int64_t len = text_bytes - off < (int64_t)MPB_BGZF_DATA ? text_bytes - off : (int64_t)MPB_BGZF_DATA;
            crc_out[m] = bgzf_crc32(text + off, (size_t)len);
        }
    };
    const int threads = n_members >= 32 ? staging_threads() : 1;
    if (threads <= 1) { run(0, n_members); return; }
    std::vector<std::thread> th;
    const int64_t per = (n_members + threads - 1) / threads;
    int64_t taken = per < n_members ? per : n_members;     // helpers take [per, taken); the rest is done here
    try {
        th.reserve((size_t)threads);
        for (int t = 1; t < threads; t++) {
            const int64_t lo = per * t, hi = lo + per < n_members ? lo + per : n_members;
            if (lo >= n_members) break;
            th.emplace_back(run, lo, hi);
            taken = hi;
        }
    } catch (...) { }                                      // no more threads to be had: this one does what is left
    run(0, per < n_members ? per : n_members);
    if (taken < n_members) run(taken, n_members);
    for (auto &t : th) t.join();
}

// ---- BGZF .gz input on the device: the validated rows (the only place a member's offsets are trusted from) ------------------------
int mpb_bgzf_member_rows(const uint8_t *in, int64_t in_len, const int64_t *offs, const int32_t *sizes, const int64_t *out_offs,
                         int64_t n, mpb_bgzf_member_row *rows_out, uint32_t *crc_out, uint8_t *why_out)
{
    if (n < 0 || in_len < 0 || !out_offs || (n > 0 && (!in || !offs || !sizes || !rows_out || !crc_out)))
        return fail(MPB_E_INVALID, "mpb_bgzf_member_rows: bad arguments");
    if (out_offs[0] < 0) return fail(MPB_E_INVALID, "mpb_bgzf_member_rows: out_offs[0] = %lld", (long long)out_offs[0]);
    for (int64_t k = 0; k < n; k++) {
        if (out_offs[k + 1] < out_offs[k])
            return fail(MPB_E_INVALID, "mpb_bgzf_member_rows: out_offs decreases at member %lld", (long long)k);
        if (offs[k] < 0 || sizes[k] < 0 || offs[k] > in_len - (int64_t)sizes[k])
            return fail(MPB_E_INVALID, "mpb_bgzf_member_rows: member %lld (offset %lld, %d bytes) does not lie inside the %lld bytes of input",
                        (long long)k, (long long)offs[k], (int)sizes[k], (long long)in_len);
    }
    for (int64_t k = 0; k < n; k++) {
        mpb_bgzf_member_row &r = rows_out[k];
        r.stream_off = 0; r.out_off = out_offs[k]; r.stream_len = 0; r.out_len = -1;
        crc_out[k] = 0;
        if (why_out) why_out[k] = MPB_BGZF_WHY_HEADER;
        const uint8_t *p = in + offs[k];
        const int64_t size = sizes[k];
        if (size < 12 + 6 + 8 || p[0] != 0x1f || p[1] != 0x8b || p[2] != 8 || p[3] != 4) continue;
        const int64_t xlen = p[10] | (p[11] << 8), xend = 12 + xlen;
        if (xend + 8 > size) continue;                       // the extra field, then at least the trailer
        int64_t bsize = -1;
        for (int64_t q = 12; q + 4 <= xend;) {               // the first 'B','C' subfield with a 2-byte value, as mio_bgzf_scan reads it
            const int64_t slen = p[q + 2] | (p[q + 3] << 8);
            if (p[q] == 'B' && p[q + 1] == 'C' && slen == 2 && q + 6 <= xend) { bsize = p[q + 4] | (p[q + 5] << 8); break; }
            q += 4 + slen;
        }
        if (bsize < 0 || bsize + 1 != size) continue;
        const uint8_t *t = p + size - 8;
        const uint32_t crc = t[0] | (t[1] << 8) | (t[2] << 16) | ((uint32_t)t[3] << 24);
        const int64_t isize = t[4] | (t[5] << 8) | (t[6] << 16) | ((int64_t)t[7] << 24);
        if (isize > 65536 || isize != out_offs[k + 1] - out_offs[k]) continue;
        r.stream_off = offs[k] + xend;
        r.stream_len = (int32_t)(size - xend - 8);
        r.out_len = (int32_t)isize;
        crc_out[k] = crc;
        if (why_out) why_out[k] = MPB_BGZF_WHY_OK;
    }
    return MPB_OK;
}

// ---- ... and what the inflating entries make of a member behind the kernel -------------------------------------------------------
uint8_t bgzf_member_reason(uint32_t status_word)
{
    return (uint8_t)(status_word <= MPB_BGZF_WHY_TRAILING_BYTES ? status_word : MPB_BGZF_WHY_HEADER);
}

void bgzf_stats_add(mpb_bgzf_inflate_stats *acc, const uint32_t *ms)
{
    acc->taken++;
    acc->stored_blocks += ms[1]; acc->fixed_blocks += ms[2]; acc->dynamic_blocks += ms[3];
    acc->literals += ms[4]; acc->matches += ms[5]; acc->matched_bytes += ms[6];
    if (acc->longest_code < (int64_t)ms[7]) acc->longest_code = (int64_t)ms[7];
}

bool bgzf_stream_range(const mpb_bgzf_member_row *rows, int64_t n, bool any, int64_t *lo, int64_t *hi)
{
    for (int64_t k = 0; k < n; k++) {
        if (rows[k].out_len < 0) continue;
        const int64_t a = rows[k].stream_off, b = a + rows[k].stream_len;
        if (!any || a < *lo) *lo = a;
        if (!any || b > *hi) *hi = b;
        any = true;
    }
    return any;
}
