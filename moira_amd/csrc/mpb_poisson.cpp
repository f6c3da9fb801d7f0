// mpb_poisson.cpp -- the Poisson approximation (SURVEY f-3) on the device, behind the C ABI of libmoira_pb.so (include/moira_pb.h):
// lambda per read (k_lambda), the CDF tail on the device (k_poisson_tail) with the host tail (mpb_hostonly.cpp) for the reads it
// hands back, the resident and host-fed entries and the per-read twin of moira.py's calculate_errors_poisson.
// (Every mpb_* function defined here has C linkage: include/moira_pb.h declares it inside extern "C".)

#include "mpb_ctx.h"

#include <cstring>
#include <new>

// ---- Poisson approximation (SURVEY f-3) ------------------------------------------------------

int mpb_poisson_lambda_device(mpb_ctx *c, const uint8_t *d_q, int64_t n, int64_t row_stride,
                              const int32_t *d_len, int32_t fixed_len, double *d_lambda, int32_t *d_ns)
{
    CTXCHK(c);
    if (n < 0 || row_stride <= 0 || row_stride % 16 != 0) return fail(MPB_E_INVALID, "bad matrix shape");
    if (row_stride > MPB_LAMBDA_MAX_STRIDE) return fail(MPB_E_INVALID, "row_stride %lld exceeds %d", (long long)row_stride, MPB_LAMBDA_MAX_STRIDE);
    if (((uintptr_t)d_q & 15) != 0) return fail(MPB_E_INVALID, "quality matrix must be 16-byte aligned");
    if (!d_len && (fixed_len < 0 || fixed_len > row_stride)) return fail(MPB_E_INVALID, "fixed_len does not fit row_stride");
    if (n == 0) return MPB_OK;
    if (!d_q || !d_lambda || !d_ns) return fail(MPB_E_INVALID, "NULL device buffer");
    int rc = ensure_workspace(c, 1);
    if (rc) return rc;
    HIPCHK(hipMemsetAsync(c->ws.ovf_count, 0, sizeof(int32_t), c->stream));
    { Span t(c, MPB_K_LAMBDA);
      mpb_launch_lambda(d_q, n, row_stride, d_len, fixed_len, c->ws.lut, d_lambda, d_ns, c->ws.ovf_count, c->stream); }
    HIPCHK(hipGetLastError());
    int32_t bad = 0;
    if ((rc = copy_sync(c, &bad, c->ws.ovf_count, sizeof(bad), hipMemcpyDeviceToHost))) return rc;
    if (bad) return fail(MPB_E_INVALID, "%d read(s) contain byte 255 ('n'): the Poisson path follows the Python reference, "
                         "which scores lower-case n as a normal base -- pack it as one", bad);
    return MPB_OK;
}

#define MPB_PT_REC_CAP 65536          // more handed-back reads than this: the arrays are fetched whole

static int check_device_tail_params(const mpb_filter_params *p, const char *who)
{
    int rc = check_params(p);
    if (rc) return rc;
    if (p->alpha < 1e-5)
        return fail(MPB_E_INVALID, "%s needs alpha >= 1e-5 (the device tail's error bound does not hold below); the exact entries -- "
                    "mpb_poisson_finish_host, mpb_filter_poisson_host without MPB_FLAG_POISSON_DEVICE_TAIL -- take any alpha", who);
    return MPB_OK;
}

// k_poisson_tail on a resident batch (queued behind whatever produced d_lambda on the context's stream), the counts fetched, the
// handed-back reads finished by the host tail and written back.  with_bad255: k_lambda ran just before; its count decides first.
static int poisson_tail_resident(mpb_ctx *c, const double *d_lambda, const int32_t *d_ns, const int32_t *d_len, int32_t fixed_len,
                                 int64_t n, const mpb_filter_params *p, double *d_ee, uint8_t *d_pass, bool with_bad255,
                                 mpb_filter_counts *counts)
{
    hipStream_t s = c->stream;
    int rc = c->pt_rec.grow(c, (int64_t)MPB_PT_REC_CAP * (int64_t)sizeof(MpbPoissonRec));
    if (rc) return rc;
    int32_t *handed = &c->pin->pt_handed, *bad = &c->pin->bad255;
    unsigned long long *kept = &c->pin->pt_kept;
    *handed = 0; *bad = 0; *kept = 0;
    HIPCHK(hipMemsetAsync(c->ws.pt_count, 0, sizeof(int32_t), s));
    HIPCHK(hipMemsetAsync(c->ws.pass_count, 0, sizeof(unsigned long long), s));
    const MpbDevParams prm = make_dev_params(p, fixed_len, 1);
    { Span t(c, MPB_K_POISSON_TAIL);
      mpb_launch_poisson_tail(d_lambda, d_ns, d_len, n, prm, d_ee, d_pass, c->ws.pt_count, (MpbPoissonRec *)c->pt_rec.p, MPB_PT_REC_CAP,
                              c->ws.pass_count, s); }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(handed, c->ws.pt_count, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (counts) HIPCHK(hipMemcpyAsync(kept, c->ws.pass_count, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    if (with_bad255) HIPCHK(hipMemcpyAsync(bad, c->ws.ovf_count, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (*bad) return fail(MPB_E_INVALID, "%d read(s) contain byte 255 ('n'): the Poisson path follows the Python reference, "
                          "which scores lower-case n as a normal base -- pack it as one", *bad);
    const int64_t h = *handed;
    int64_t host_pass = 0;
    if (h > 0) {
        try {
            if (h <= MPB_PT_REC_CAP) {
                // few: their records in one copy, the host tail, their results in one copy and a scatter
                std::vector<MpbPoissonRec> rec((size_t)h);
                if ((rc = copy_sync(c, rec.data(), c->pt_rec.p, (size_t)h * sizeof(MpbPoissonRec), hipMemcpyDeviceToHost))) return rc;
                std::vector<double> lam((size_t)h), e((size_t)h);
                std::vector<int32_t> nsv((size_t)h), lv((size_t)h);
                std::vector<uint8_t> ps((size_t)h);
                for (int64_t k = 0; k < h; k++) { lam[k] = rec[k].lambda; nsv[k] = rec[k].ns; lv[k] = rec[k].len; }
                if ((rc = mpb_poisson_finish_host(lam.data(), nsv.data(), lv.data(), 0, h, p, e.data(), ps.data()))) return rc;
                std::vector<MpbPoissonFix> fix((size_t)h);
                for (int64_t k = 0; k < h; k++) { fix[k].ee = e[k]; fix[k].idx = rec[k].idx; fix[k].pass = ps[k]; host_pass += ps[k]; }
                // (`fix` is waited for before anything can return: the errors are looked at after the synchronisation)
                const hipError_t e_copy = hipMemcpyAsync(c->pt_rec.p, fix.data(), (size_t)h * sizeof(MpbPoissonFix), hipMemcpyHostToDevice, s);
                mpb_launch_poisson_patch((const MpbPoissonFix *)c->pt_rec.p, (int32_t)h, d_ee, d_pass, s);
                const hipError_t e_launch = hipGetLastError(), e_sync = hipStreamSynchronize(s);
                HIPCHK_KEPT("hipMemcpyAsync", e_copy);
                HIPCHK_KEPT("k_poisson_patch launch", e_launch);
                HIPCHK_KEPT("hipStreamSynchronize", e_sync);
            } else {
                // a large share of the batch: the arrays whole, both ways (never a copy per read)
                std::vector<double> e((size_t)n);
                std::vector<int32_t> nsv((size_t)n), lv(d_len ? (size_t)n : 0);
                std::vector<uint8_t> ps((size_t)n);
                // (one synchronisation for the group, and the errors looked at after it: the vectors outlive every copy)
                hipError_t e_copy = hipMemcpyAsync(e.data(), d_ee, (size_t)n * 8, hipMemcpyDeviceToHost, s);
                if (e_copy == hipSuccess) e_copy = hipMemcpyAsync(nsv.data(), d_ns, (size_t)n * 4, hipMemcpyDeviceToHost, s);
                if (e_copy == hipSuccess) e_copy = hipMemcpyAsync(ps.data(), d_pass, (size_t)n, hipMemcpyDeviceToHost, s);
                if (e_copy == hipSuccess && d_len) e_copy = hipMemcpyAsync(lv.data(), d_len, (size_t)n * 4, hipMemcpyDeviceToHost, s);
                hipError_t e_sync = hipStreamSynchronize(s);
                HIPCHK_KEPT("hipMemcpyAsync", e_copy);
                HIPCHK_KEPT("hipStreamSynchronize", e_sync);
                std::vector<uint8_t> was(ps);
                int64_t marked = 0;
                if ((rc = poisson_finish_marked(p, nsv.data(), d_len ? lv.data() : nullptr, fixed_len, n, e.data(), ps.data(), &marked))) return rc;
                if (marked != h) return fail(MPB_E_HIP, "k_poisson_tail counted %lld handed-back reads, %lld are marked", (long long)h, (long long)marked);
                for (int64_t i = 0; i < n; i++) if (was[i] == 2) host_pass += ps[i];
                e_copy = hipMemcpyAsync(d_ee, e.data(), (size_t)n * 8, hipMemcpyHostToDevice, s);
                if (e_copy == hipSuccess) e_copy = hipMemcpyAsync(d_pass, ps.data(), (size_t)n, hipMemcpyHostToDevice, s);
                e_sync = hipStreamSynchronize(s);
                HIPCHK_KEPT("hipMemcpyAsync", e_copy);
                HIPCHK_KEPT("hipStreamSynchronize", e_sync);
            }
        } catch (const std::bad_alloc &) {
            return fail(MPB_E_NOMEM, "out of host memory for the reads handed back to the host tail");
        }
    }
    if (counts) {
        counts->n_reads = n; counts->n_pass = (int64_t)*kept + host_pass; counts->n_fail = n - counts->n_pass; counts->n_overflow = h;
    }
    return MPB_OK;
}

int mpb_poisson_finish_device(mpb_ctx *c, const double *d_lambda, const int32_t *d_ns, const int32_t *d_len, int32_t fixed_len,
                              int64_t n, const mpb_filter_params *params, double *d_ee, uint8_t *d_pass, mpb_filter_counts *counts)
{
    CTXCHK(c);
    int rc = check_device_tail_params(params, "mpb_poisson_finish_device");
    if (rc) return rc;
    if (n < 0) return fail(MPB_E_INVALID, "n < 0");
    if (n > 0x7fffffffll - 4096) return fail(MPB_E_INVALID, "batch of %lld reads exceeds 2^31; split it", (long long)n);
    if (!d_len && fixed_len < 0) return fail(MPB_E_INVALID, "fixed_len < 0");
    if (counts) { counts->n_reads = n; counts->n_pass = 0; counts->n_fail = 0; counts->n_overflow = 0; }
    if (n == 0) return MPB_OK;
    if (!d_lambda || !d_ns || !d_ee || !d_pass) return fail(MPB_E_INVALID, "NULL device buffer");
    if ((rc = ensure_workspace(c, 1))) return rc;
    return poisson_tail_resident(c, d_lambda, d_ns, d_len, fixed_len, n, params, d_ee, d_pass, false, counts);
}

int mpb_filter_poisson_device(mpb_ctx *c, const uint8_t *d_q, int64_t n, int64_t row_stride, const int32_t *d_len, int32_t fixed_len,
                              const mpb_filter_params *params, double *d_ee, int32_t *d_ns, uint8_t *d_pass, double *d_lambda,
                              mpb_filter_counts *counts)
{
    CTXCHK(c);
    int rc = check_device_tail_params(params, "mpb_filter_poisson_device");
    if (rc) return rc;
    // (the argument checks of mpb_poisson_lambda_device)
    if (n < 0 || row_stride <= 0 || row_stride % 16 != 0) return fail(MPB_E_INVALID, "bad matrix shape");
    if (n > 0x7fffffffll - 4096) return fail(MPB_E_INVALID, "batch of %lld reads exceeds 2^31; split it", (long long)n);
    if (row_stride > MPB_LAMBDA_MAX_STRIDE) return fail(MPB_E_INVALID, "row_stride %lld exceeds %d", (long long)row_stride, MPB_LAMBDA_MAX_STRIDE);
    if (((uintptr_t)d_q & 15) != 0) return fail(MPB_E_INVALID, "quality matrix must be 16-byte aligned");
    if (!d_len && (fixed_len < 0 || fixed_len > row_stride)) return fail(MPB_E_INVALID, "fixed_len does not fit row_stride");
    if (counts) { counts->n_reads = n; counts->n_pass = 0; counts->n_fail = 0; counts->n_overflow = 0; }
    if (n == 0) return MPB_OK;
    if (!d_q || !d_ee || !d_ns || !d_pass) return fail(MPB_E_INVALID, "NULL device buffer");
    if ((rc = ensure_workspace(c, 1))) return rc;
    double *lam = d_lambda ? d_lambda : d_ee;        // without d_lambda, lambda lives in d_ee until the tail overwrites it
    HIPCHK(hipMemsetAsync(c->ws.ovf_count, 0, sizeof(int32_t), c->stream));
    { Span t(c, MPB_K_LAMBDA);
      mpb_launch_lambda(d_q, n, row_stride, d_len, fixed_len, c->ws.lut, lam, d_ns, c->ws.ovf_count, c->stream); }
    HIPCHK(hipGetLastError());
    return poisson_tail_resident(c, lam, d_ns, d_len, fixed_len, n, params, d_ee, d_pass, true, counts);
}

int mpb_filter_poisson_host(mpb_ctx *c, const uint8_t *q, int64_t n, int64_t row_stride, const int32_t *len,
                            int32_t fixed_len, const mpb_filter_params *params, double *ee, int32_t *ns,
                            uint8_t *pass, mpb_filter_counts *counts)
{
    CTXCHK(c);
    int rc = (params && (params->flags & MPB_FLAG_POISSON_DEVICE_TAIL)) ? check_device_tail_params(params, "MPB_FLAG_POISSON_DEVICE_TAIL")
                                                                        : check_params(params);
    if (rc) return rc;
    if (n < 0 || row_stride <= 0 || row_stride % 16 != 0) return fail(MPB_E_INVALID, "bad matrix shape");
    if (row_stride > MPB_LAMBDA_MAX_STRIDE) return fail(MPB_E_INVALID, "row_stride %lld exceeds %d", (long long)row_stride, MPB_LAMBDA_MAX_STRIDE);
    if (n > 0 && (!q || !ee || !ns || !pass)) return fail(MPB_E_INVALID, "NULL host buffer");
    if (!len && (fixed_len < 0 || fixed_len > row_stride)) return fail(MPB_E_INVALID, "fixed_len does not fit row_stride");
    if (len)
        for (int64_t i = 0; i < n; i++)
            if (len[i] < 0 || len[i] > row_stride)
                return fail(MPB_E_INVALID, "read %lld: length %d does not fit the %lld-byte row", (long long)i, len[i], (long long)row_stride);
    if (counts) { counts->n_reads = n; counts->n_pass = 0; counts->n_fail = 0; counts->n_overflow = 0; }
    if (n == 0) return MPB_OK;
    // the same four-slot pipeline as mpb_filter_host: H2D of chunk k+1 | k_lambda of chunk k | D2H of chunk k-1, and the
    // scalar tail of a chunk runs on the host while the GPU is busy with the chunks after it
    // MPB_FLAG_POISSON_DEVICE_TAIL: k_poisson_tail runs on each chunk behind k_lambda, the host tail only on the reads it hands back
    return filter_host_pipeline(c, q, n, row_stride, len, fixed_len, params, ee, ns, pass, counts,
                                (params->flags & MPB_FLAG_POISSON_DEVICE_TAIL) ? 2 : 1);
}

// One read, the twin of moira.py's calculate_errors_poisson(sequence, quals, alpha) -> (expected_errors, Ns)
// (moira/moira.py:1637-1679): any non-negative int is a score (see pack_one_read), 'n' is a base, Q0 is p = 1.
// ee is NaN where the Python function raises OverflowError (Lambda ** j or the factorial leave the float range).
int mpb_calculate_errors_poisson(mpb_ctx *c, const char *sequence, const int32_t *quals, int32_t len, double alpha,
                                 double *ee, int32_t *ns)
{
    CTXCHK(c);
    if (!ee || !ns) return fail(MPB_E_INVALID, "NULL output");
    if (!(alpha > 0 && alpha < 1)) return fail(MPB_E_INVALID, "Alpha must be between 0 and 1");
    if (len < 0 || (len > 0 && !quals)) return fail(MPB_E_INVALID, "bad arguments");
    if (sequence && (int32_t)strlen(sequence) != len) return fail(MPB_E_INVALID, "sequence and quals must have the same length");
    const int32_t stride = (int32_t)align_up(len > 0 ? len : 1, 16);
    std::vector<uint8_t> row((size_t)stride);
    const mpb_filter_params prm = per_read_params(alpha);
    uint8_t pass = 0;
    bool priv = false;
    double2 h[256];
    int rc = mpbi_pack_one_read(sequence, quals, len, true, row.data(), stride, h, &priv);
    if (rc) return rc;
    PrivateTable guard(c);
    if (priv && (rc = guard.install(h)) != MPB_OK) return rc;
    return mpb_filter_poisson_host(c, row.data(), 1, stride, nullptr, len, &prm, ee, ns, &pass, nullptr);
}
