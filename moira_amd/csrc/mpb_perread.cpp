// mpb_perread.cpp -- the per-read path of the C ABI of libmoira_pb.so (include/moira_pb.h): mpb_calculate_errors_PB, the resident
// one-read server behind it (k_serve with one mailbox entry), and the mpbi_* hooks of the broker (mpb_host_internal.h).
// (Every mpb_* and mpbi_* function defined here has C linkage: include/moira_pb.h and mpb_host_internal.h declare them so.)

#include "mpb_ctx.h"

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <unistd.h>

// argument rules of the per-read entry (moira/bernoullimodule.c:79-90), shared with the broker's client side
int mpbi_check_one_read(const char *contig, const int32_t *contig_quals, int32_t len, double alpha, const void *ee, const void *ns)
{
    if (!ee || !ns) return fail(MPB_E_INVALID, "NULL output");
    if (!(alpha > 0 && alpha < 1)) return fail(MPB_E_INVALID, "Alpha must be between 0 and 1");   // bernoullimodule.c:79-83
    if (len < 0 || (len > 0 && !contig_quals)) return fail(MPB_E_INVALID, "bad arguments");
    if (contig && (int32_t)strlen(contig) != len)                                               // bernoullimodule.c:85-90
        return fail(MPB_E_INVALID, "contig and contig_quals must have the same length");
    if (len > MPB_MAX_LEN) return fail(MPB_E_INVALID, "reads longer than %d bases are not supported", MPB_MAX_LEN);
    return MPB_OK;
}

// ---- the per-read entry without a launch per call (round 5) ----------------------------------------------------------
// mpb_calculate_errors_PB from a process of its own (moira.py --processors 1: one call per read) paid a k_small launch per
// call: 26 us of which the kernel is 12.  While such calls keep coming the context keeps k_serve resident with ONE mailbox
// entry (mpb_kernels.hip; the broker's form has one per slot): the call writes row + parameters + door word into pinned
// memory and spins on done[0].  The kernel leaves by itself 100 ms after its launch -- so 100 ms after the last call at
// the latest -- and the next call launches it again.  Anything that frees device or pinned memory (a device-wide wait in the
// runtime) asks it to leave first.  MPB_SERVE=0 keeps the launch per call.
static inline int64_t mono_us()
{
    timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (int64_t)ts.tv_sec * 1000000 + ts.tv_nsec / 1000;
}

void serve_quiesce(mpb_ctx *c)
{
    auto &sv = c->serve;
    if (!sv.ok || !sv.running) return;
    __atomic_store_n((uint32_t *)sv.box.stop, 1u, __ATOMIC_SEQ_CST);
    (void)hipStreamSynchronize(sv.stream);
    __atomic_store_n((uint32_t *)sv.box.stop, 0u, __ATOMIC_SEQ_CST);
    sv.running = false;
}

void serve_free(mpb_ctx *c)
{
    auto &sv = c->serve;
    serve_quiesce(c);
    if (sv.stream) (void)hipStreamDestroy(sv.stream);
    sv.stream = nullptr;
    sv.pin.release();
    sv.dev.release();
    sv.ok = false;
}

static bool serve_init(mpb_ctx *c)
{
    auto &sv = c->serve;
    if (sv.tried) return sv.ok;
    sv.tried = true;
    const char *e = getenv("MPB_SERVE");
    if (e && atoi(e) == 0) return false;
    MpbServeBox &x = sv.box;
    // pinned: row | parameters | door | done | ee | ns | pass | stop | exited; device: the parked row and what the class body reads
    auto pinned = [&x](Carver &k) {
        k.take(x.q, MPB_SERVE_STRIDE); k.take(x.prm, 1); k.take(x.door, 1); k.take(x.done, 1); k.take(x.ee, 1); k.take(x.ns, 1);
        k.take(x.pass, 1); k.take(x.stop, 1); k.take(x.exited, 1);
    };
    auto device = [&x](Carver &k) {
        k.take(x.stage, MPB_SERVE_STRIDE + 256); k.take(x.ns_dev, 1); k.take(x.cls, 1); k.take(x.ident, 1); k.take(x.gone, 1);
    };
    Carver pin_size, dev_size;
    pinned(pin_size);
    device(dev_size);
    if (hipStreamCreateWithFlags(&sv.stream, hipStreamNonBlocking) != hipSuccess ||
        sv.pin.alloc(pin_size.bytes()) != hipSuccess || sv.dev.alloc(dev_size.bytes()) != hipSuccess ||
        hipMemset(sv.dev.p, 0, (size_t)dev_size.bytes()) != hipSuccess) {
        (void)hipGetLastError();
        if (sv.stream) (void)hipStreamDestroy(sv.stream);
        sv.pin.release();
        sv.dev.release();
        sv.stream = nullptr;
        return false;                                   // the launch per call remains (the box's pointers are null)
    }
    memset(sv.pin.p, 0, (size_t)pin_size.bytes());
    Carver pin_place(sv.pin.p), dev_place(sv.dev.p);
    pinned(pin_place);
    device(dev_place);
    x.stride = MPB_SERVE_STRIDE;
    x.q_step = MPB_SERVE_STRIDE; x.prm_step = sizeof(MpbServePrm); x.door_step = 8; x.done_step = 4; x.ee_step = 8; x.ns_step = 4; x.pass_step = 1;
    x.n_ent = 1;
    sv.ok = true;
    return true;
}

static int serve_launch(mpb_ctx *c)
{
    auto &sv = c->serve;
    if (++sv.generation == 0) sv.generation = 1;
    mpb_launch_serve(sv.box, c->d_lut, sv.generation, 100, sv.stream);
    HIPCHK(hipGetLastError());
    sv.running = true;
    return MPB_OK;
}

// one packed read (default table, at most MPB_SERVE_STRIDE - 1 bases) through the resident server; *served = false: not
// taken (no server, or the read missed its row budget there): the caller goes the ordinary way
static int serve_one(mpb_ctx *c, const uint8_t *row, int32_t len, double alpha, double *ee, int32_t *ns, bool *served)
{
    *served = false;
    if (!serve_init(c)) return MPB_OK;
    auto &sv = c->serve;
    const MpbServeBox &x = sv.box;
    if (sv.running && __atomic_load_n(x.exited, __ATOMIC_ACQUIRE) == sv.generation) sv.running = false;
    memcpy((void *)x.q, row, (size_t)((len + 15) & ~15));
    if (alpha != sv.cached_alpha) { mpbi_small_params(alpha, &sv.cached_prm); sv.cached_alpha = alpha; }
    ((MpbServePrm *)x.prm)->p = sv.cached_prm;
    if (++sv.tok == 0) sv.tok = 1;
    __atomic_store_n((unsigned long long *)x.door, ((unsigned long long)(uint32_t)len << 32) | sv.tok, __ATOMIC_RELEASE);
    int rc;
    if (!sv.running && (rc = serve_launch(c))) return rc;
    const int64_t t0 = mono_us();
    int64_t asked = t0;
    for (unsigned spins = 0;; spins++) {
        if (__atomic_load_n(x.done, __ATOMIC_ACQUIRE) == sv.tok) break;
        __builtin_ia32_pause();
        if ((spins & 1023u) != 1023u) continue;
        // a wave that left just before the door word arrived: the launch that follows serves it (it starts from done[0])
        if (__atomic_load_n(x.exited, __ATOMIC_ACQUIRE) == sv.generation) {
            if (__atomic_load_n(x.done, __ATOMIC_ACQUIRE) == sv.tok) break;
            if ((rc = serve_launch(c))) return rc;
        }
        // a GPU that is busy with somebody else's long kernel answers late, as a launch per call would: wait (off the CPU
        // between looks after two milliseconds), and ask the runtime every two seconds -- only a fault ends the wait
        const int64_t now = mono_us();
        if (now - t0 > 2000) usleep(50);
        if (now - asked > 2000000) {
            asked = now;
            const hipError_t q = hipStreamQuery(sv.stream);
            if (q != hipSuccess && q != hipErrorNotReady) {
                sv.running = false;
                return fail(MPB_E_HIP, "the resident per-read kernel failed: %s", hipGetErrorString(q));
            }
        }
    }
    if (*x.pass == 2) return MPB_OK;                    // row budget missed / a wide read: the ordinary path
    *ee = *x.ee;
    *ns = *x.ns;
    *served = true;
    return MPB_OK;
}

int mpbi_pack_one_read(const char *contig, const int32_t *quals, int32_t len, bool poisson, uint8_t *row, int32_t row_bytes,
                       double2 *h, bool *priv)
{
    return pack_one_read(contig, quals, len, poisson, row, row_bytes, (MpbPair *)h, priv);
}

// one packed row (and, when the read carries scores above 254, its private table h) -> (ee, Ns): the GPU half of the
// per-read entry.  The broker calls it for the reads it cannot put into a micro-batch.
int mpbi_run_packed_read(mpb_ctx *c, const uint8_t *row, int32_t len, int32_t stride, const double2 *h, double alpha,
                         double *ee, int32_t *ns)
{
    const mpb_filter_params prm = per_read_params(alpha);
    uint8_t pass = 0;
    PrivateTable guard(c);
    int rc;
    if (h && (rc = guard.install(h)) != MPB_OK) return rc;
    return mpb_filter_host(c, row, 1, stride, nullptr, len, &prm, ee, ns, &pass, nullptr);
}

int mpb_calculate_errors_PB(mpb_ctx *c, const char *contig, const int32_t *contig_quals, int32_t len,
                            double alpha, double *ee, int32_t *ns)
{
    CTXCHK(c);
    int rc = mpbi_check_one_read(contig, contig_quals, len, alpha, ee, ns);
    if (rc) return rc;
    const int32_t stride = (int32_t)align_up(len > 0 ? len : 1, 16);
    std::vector<uint8_t> row((size_t)stride);
    bool priv = false;
    double2 h[256];
    if ((rc = mpbi_pack_one_read(contig, contig_quals, len, false, row.data(), stride, h, &priv))) return rc;
    if (!priv && len <= MPB_SERVE_STRIDE - 1 && !c->timing) {
        bool served = false;
        if ((rc = serve_one(c, row.data(), len, alpha, ee, ns, &served)) || served) return rc;
    }
    return mpbi_run_packed_read(c, row.data(), len, stride, priv ? h : nullptr, alpha, ee, ns);
}

// One micro-batch of the broker: m packed rows that already lie in device memory -> one k_small launch on stream s
// (one read per wave), results into device arrays.  Nothing here synchronises; a read that misses its row budget comes
// back with pass == 2 and the broker re-runs it alone.  cls / ident are the launch's own scratch (m bytes / m int32),
// so that several micro-batches can be in flight on different streams.
int mpbi_small_async(mpb_ctx *c, const uint8_t *d_q, int64_t m, int64_t stride, const int32_t *d_len, double alpha,
                     double *d_ee, int32_t *d_ns, uint8_t *d_pass, uint8_t *d_cls, int32_t *d_ident, hipStream_t s,
                     const MpbSmallHost *host)
{
    const mpb_filter_params prm = per_read_params(alpha);
    const int32_t max_len = (int32_t)(stride < MPB_MAX_LEN ? stride : MPB_MAX_LEN);
    const MpbDevParams dp = make_dev_params(&prm, 0, max_len);
    int rc = ensure_workspace(c, m);               // (the broker sizes it once, before anything is in flight)
    if (rc) return rc;
    MpbWorkspace ws = c->ws;                       // only lut / cls / perm are read by the launch
    ws.lut = c->d_lut;
    ws.cls = d_cls;
    ws.perm = d_ident;
    mpb_launch_small(d_q, m, stride, d_len, dp, ws, d_ns, d_ee, d_pass, s, host);
    HIPCHK(hipGetLastError());
    return MPB_OK;
}

void mpbi_small_params(double alpha, MpbDevParams *out)
{
    const mpb_filter_params prm = per_read_params(alpha);
    *out = make_dev_params(&prm, 0, MPB_SERVE_STRIDE);
}

int mpbi_serve_launch(mpb_ctx *c, const MpbServeBox *box, uint32_t generation, uint32_t lifetime_ms, hipStream_t s)
{
    mpb_launch_serve(*box, c->d_lut, generation, lifetime_ms, s);
    HIPCHK(hipGetLastError());
    return MPB_OK;
}

int mpbi_ctx_device(const mpb_ctx *c) { return c ? c->device : -1; }

int mpbi_fail(int code, const char *msg) { return fail(code, "%s", msg); }
