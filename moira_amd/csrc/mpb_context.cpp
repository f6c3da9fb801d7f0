// mpb_context.cpp -- the context of the C ABI of libmoira_pb.so (include/moira_pb.h): its life cycle, the device tables, stream
// and memory entries, the owner of its growable blocks (Buf, mpb_ctx.h) and the workspaces carved from them, kernel timing.
// (Every mpb_* function defined here has C linkage: include/moira_pb.h declares it inside extern "C".)

#include "mpb_ctx.h"

#include <cstring>
#include <new>

// ---- blocks --------------------------------------------------------------------------------------

hipError_t Buf::alloc(int64_t bytes)
{
    const hipError_t e = kind == BUF_DEVICE ? hipMalloc(&p, (size_t)bytes)
                                            : hipHostMalloc(&p, (size_t)bytes, kind == BUF_MAPPED ? hipHostMallocMapped : hipHostMallocDefault);
    if (e != hipSuccess) p = nullptr;
    cap = p ? bytes : 0;
    return e;
}

void Buf::release()
{
    if (p) (void)(kind == BUF_DEVICE ? hipFree(p) : hipHostFree(p));
    p = nullptr;
    cap = 0;
}

int Buf::grow(mpb_ctx *c, int64_t bytes, int64_t alloc_bytes)
{
    if (bytes <= cap) return MPB_OK;
    HIPCHK(hipStreamSynchronize(c->stream));
    serve_quiesce(c);
    void *old = p;
    p = nullptr;
    cap = 0;
    if (old) HIPCHK(kind == BUF_DEVICE ? hipFree(old) : hipHostFree(old));
    HIPCHK(alloc(alloc_bytes > bytes ? alloc_bytes : bytes));
    return MPB_OK;
}

int copy_sync(mpb_ctx *c, void *dst, const void *src, size_t bytes, hipMemcpyKind kind)
{
    const hipError_t e_copy = hipMemcpyAsync(dst, src, bytes, kind, c->stream);
    const hipError_t e_sync = hipStreamSynchronize(c->stream);
    HIPCHK_KEPT("hipMemcpyAsync", e_copy);
    HIPCHK_KEPT("hipStreamSynchronize", e_sync);
    return MPB_OK;
}

// ---- life cycle ------------------------------------------------------------------------------------

int mpb_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int mpb_create(int device_id, mpb_ctx **out)
{
    if (!out) return fail(MPB_E_INVALID, "mpb_create: out is NULL");
    *out = nullptr;
    int n = mpb_device_count();
    if (n <= 0) return fail(MPB_E_NODEVICE, "no HIP device visible (this library has no CPU path)");
    if (device_id < 0 || device_id >= n)
        return fail(MPB_E_NODEVICE, "device %d out of range (0..%d)", device_id, n - 1);
    HIPCHK(hipSetDevice(device_id));
    mpb_ctx *c = new (std::nothrow) mpb_ctx();
    if (!c) return fail(MPB_E_NOMEM, "host allocation failed");
    c->device = device_id;
    hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->out_stream, hipStreamNonBlocking);
    for (int k = 0; k < MPB_HOST_SLOTS && e == hipSuccess; k++) {
        e = hipEventCreateWithFlags(&c->slot[k].h2d_done, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&c->slot[k].k_done, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&c->slot[k].d2h_done, hipEventDisableTiming);
    }
    c->copy_threads = staging_threads();
    auto tables = [c](Carver &k) { k.take(c->d_lut, 256); k.take(c->d_lut_odds, 256); k.take(c->d_lut_private, 256); };
    Carver size;
    tables(size);
    if (e == hipSuccess) e = c->luts.alloc(size.bytes());
    if (e == hipSuccess) {
        Carver place(c->luts.p);
        tables(place);
        MpbPair both[2][256], (&h)[256] = both[0];       // the table and its odds twin, back to back as in the block
        build_lut(both[0], both[1]);
        // the narrow pass keeps {p'} alone and recomputes 1 - p' on the device: only sound if the table's a IS that difference
        // (it is: p' == p bit for bit for every encodable score, tests/test_oracle_golden.py::test_lut_pins)
        c->narrow_ok = true;
        for (int qq = 1; qq < 255; qq++) {
            volatile double d = 1.0 - h[qq].y;
            if (memcmp((const void *)&d, &h[qq].x, sizeof(double)) != 0) c->narrow_ok = false;
        }
        e = hipMemcpyAsync(c->d_lut, both, sizeof(both), hipMemcpyHostToDevice, c->stream);
        const hipError_t e_sync = hipStreamSynchronize(c->stream);  // `both` is on this frame: waited for whatever the copy said
        if (e == hipSuccess) e = e_sync;
    }
    if (e == hipSuccess) e = c->pin_mem.alloc(sizeof(PinWords));
    c->pin = (PinWords *)c->pin_mem.p;
    if (e == hipSuccess) {
        hipDeviceProp_t prop;
        e = hipGetDeviceProperties(&prop, device_id);
        if (e == hipSuccess) c->n_cu = prop.multiProcessorCount;
    }
    if (e != hipSuccess) {
        int rc = fail(MPB_E_HIP, "context setup failed: %s", hipGetErrorString(e));
        mpb_destroy(c);
        return rc;
    }
    *out = c;
    return MPB_OK;
}

int mpb_destroy(mpb_ctx *c)
{
    if (!c) return MPB_OK;
    (void)hipSetDevice(c->device);
    serve_free(c);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->copy_stream) (void)hipStreamSynchronize(c->copy_stream);
    if (c->out_stream) (void)hipStreamSynchronize(c->out_stream);
    for (auto &sl : c->slot) {
        if (sl.h2d_done) (void)hipEventDestroy(sl.h2d_done);
        if (sl.k_done) (void)hipEventDestroy(sl.k_done);
        if (sl.d2h_done) (void)hipEventDestroy(sl.d2h_done);
    }
    for (auto &s : c->spans) { (void)hipEventDestroy(s.a); (void)hipEventDestroy(s.b); }
    for (auto ev : c->event_pool) (void)hipEventDestroy(ev);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    if (c->copy_stream) (void)hipStreamDestroy(c->copy_stream);
    if (c->out_stream) (void)hipStreamDestroy(c->out_stream);
    delete c;                            // every Buf releases its block
    return MPB_OK;
}

int mpb_device_lut(mpb_ctx *c, double *a_out, double *b_out)
{
    CTXCHK(c);
    if (!a_out || !b_out) return fail(MPB_E_INVALID, "mpb_device_lut: NULL output");
    double2 h[256];
    int rc = copy_sync(c, h, c->d_lut, sizeof(h), hipMemcpyDeviceToHost);
    if (rc) return rc;
    for (int q = 0; q < 256; q++) { a_out[q] = h[q].x; b_out[q] = h[q].y; }
    return MPB_OK;
}

int mpb_stream(mpb_ctx *c, void **stream_out)
{
    CTXCHK(c);
    if (!stream_out) return fail(MPB_E_INVALID, "stream_out is NULL");
    *stream_out = (void *)c->stream;
    return MPB_OK;
}

int mpb_synchronize(mpb_ctx *c)
{
    CTXCHK(c);
    HIPCHK(hipStreamSynchronize(c->stream));
    return MPB_OK;
}

int mpb_malloc(mpb_ctx *c, int64_t bytes, void **dptr_out)
{
    CTXCHK(c);
    if (!dptr_out || bytes < 0) return fail(MPB_E_INVALID, "mpb_malloc: bad arguments");
    *dptr_out = nullptr;
    HIPCHK(hipMalloc(dptr_out, bytes > 0 ? (size_t)bytes : 16));
    return MPB_OK;
}

int mpb_free(mpb_ctx *c, void *dptr)
{
    CTXCHK(c);
    HIPCHK(hipStreamSynchronize(c->stream));
    serve_quiesce(c);
    if (dptr) HIPCHK(hipFree(dptr));
    return MPB_OK;
}

int mpb_memcpy_h2d(mpb_ctx *c, void *dst, const void *src, int64_t bytes)
{
    CTXCHK(c);
    if (bytes < 0 || (bytes > 0 && (!dst || !src))) return fail(MPB_E_INVALID, "mpb_memcpy_h2d: bad arguments");
    if (bytes == 0) return MPB_OK;
    return copy_sync(c, dst, src, (size_t)bytes, hipMemcpyHostToDevice);
}

int mpb_memcpy_d2h(mpb_ctx *c, void *dst, const void *src, int64_t bytes)
{
    CTXCHK(c);
    if (bytes < 0 || (bytes > 0 && (!dst || !src))) return fail(MPB_E_INVALID, "mpb_memcpy_d2h: bad arguments");
    if (bytes == 0) return MPB_OK;
    return copy_sync(c, dst, src, (size_t)bytes, hipMemcpyDeviceToHost);
}

int mpb_memset(mpb_ctx *c, void *dst, int value, int64_t bytes)
{
    CTXCHK(c);
    if (bytes < 0 || (bytes > 0 && !dst)) return fail(MPB_E_INVALID, "mpb_memset: bad arguments");
    if (bytes == 0) return MPB_OK;
    HIPCHK(hipMemsetAsync(dst, value, (size_t)bytes, c->stream));
    return MPB_OK;
}

int mpb_host_alloc(mpb_ctx *c, int64_t bytes, void **hptr_out)
{
    CTXCHK(c);
    if (!hptr_out || bytes < 0) return fail(MPB_E_INVALID, "mpb_host_alloc: bad arguments");
    *hptr_out = nullptr;
    HIPCHK(hipHostMalloc(hptr_out, bytes > 0 ? (size_t)bytes : 16, hipHostMallocDefault));
    return MPB_OK;
}

int mpb_host_free(mpb_ctx *c, void *hptr)
{
    CTXCHK(c);
    drain_pipeline(c);
    serve_quiesce(c);
    if (hptr) HIPCHK(hipHostFree(hptr));
    return MPB_OK;
}

// ---- workspace ---------------------------------------------------------------------------------

int ensure_workspace(mpb_ctx *c, int64_t n)
{
    if (!c->ws_small.p) {
        int rc = c->ws_small.grow(c, sizeof(MpbSmallBlock));
        if (rc) return rc;
        // on the context's stream, not the null stream: the stream is non-blocking, so a null-stream
        // memset is unordered with the kernels below and can land after they have written the tables
        HIPCHK(hipMemsetAsync(c->ws_small.p, 0, sizeof(MpbSmallBlock), c->stream));
        MpbSmallBlock *b = (MpbSmallBlock *)c->ws_small.p;
        c->ws.tables = &b->tables;
        c->ws.tables2 = &b->tables2;
        c->ws.ovf_count = &b->ovf_count;
        c->ws.bad_len = &b->bad_len;
        c->ws.pass_count = &b->pass_count;
        c->ws.ovf_total = &b->ovf_total;
        c->ws.wide_count = &b->wide_count;
        c->ws.alg_cells = &b->alg_cells;
        c->ws.nar_count = &b->nar_count;
        c->ws.nar_sample = b->nar_sample;
        c->ws.pt_count = &b->pt_count;
        c->ws.lut = c->d_lut;
    }
    if (n <= c->ws_cap) return MPB_OK;
    c->ws_cap = 0;
    const int64_t cap = n + n / 8 + 1024;
    const int64_t nb = (cap + MPB_PRE_READS - 1) / MPB_PRE_READS;
    MpbWorkspace &w = c->ws;
    int rc = carve(c, c->ws_block, [&w, cap, nb](Carver &k) {
        k.take(w.cls, cap);
        k.take(w.perm, cap + (int64_t)MPB_NCLS * 64);
        k.take(w.perm_ns, cap + (int64_t)MPB_NCLS * 64);
        k.take(w.blockhist, nb * MPB_SKEYS);
        k.take(w.ovf_list, cap);
    });
    if (rc) return rc;
    c->ws_cap = cap;
    return MPB_OK;
}

// the wide-read list of a batch whose rows can hold more than MPB_TILE_MAX_ROWS - 1 bases (8 bytes per read)
int ensure_wide_workspace(mpb_ctx *c, int64_t n)
{
    if (n <= c->ws_wide_cap) return MPB_OK;
    c->ws_wide_cap = 0;
    const int64_t cap = n + n / 8 + 1024;
    MpbWorkspace &w = c->ws;
    int rc = carve(c, c->ws_wide, [&w, cap](Carver &k) { k.take(w.wide_list, cap); k.take(w.wide_rows, cap); });
    if (rc) return rc;
    c->ws_wide_cap = cap;
    return MPB_OK;
}

// the lists of the natural-order narrow pass (round 5; mpb_internal.h) and, for ragged batches, its order entries and group costs
int ensure_narrow_workspace(mpb_ctx *c, int64_t n, bool ragged)
{
    const int64_t cap = n + n / 8 + 1024;
    MpbWorkspace &w = c->ws;
    int rc;
    if (n > c->ws_nar_cap) {
        c->ws_nar_cap = 0;
        rc = carve(c, c->ws_nar, [&w, cap](Carver &k) {
            k.take(w.nar_seg, cap + 64);
            k.take(w.nar_list, cap + 64);
            k.take(w.nar_wave_count, MPB_NAR_MAX_WAVES + 1);
        });
        if (rc) return rc;
        c->ws_nar_cap = cap;
    }
    if (ragged && n > c->ws_rg_cap) {
        c->ws_rg_cap = 0;
        rc = carve(c, c->ws_rg, [&w, cap](Carver &k) {
            k.take(w.rg_ord, cap + 64);
            k.take(w.rg_gpre, cap / 64 + 2);
            k.take(w.rg_wsum, cap / 4096 + 2);
            k.take(w.rg_wpre, cap / 4096 + 2);
            k.take(w.rg_gstart, MPB_NAR_MAX_WAVES + 1);
        });
        if (rc) return rc;
        c->ws_rg_cap = cap;
        if (!c->rg_per_cu[0]) mpb_narrow_rg_blocks_per_cu(c->rg_per_cu);
    }
    return MPB_OK;
}

int PrivateTable::install(const double2 *h)
{
    int rc = ensure_workspace(c, 1);
    if (rc) return rc;
    if ((rc = copy_sync(c, c->d_lut_private, h, 256 * sizeof(double2), hipMemcpyHostToDevice))) return rc;   // h lives on the caller's stack
    c->ws.lut = c->d_lut_private;
    on = true;
    return MPB_OK;
}

// ---- timing ------------------------------------------------------------------------------------

static hipEvent_t get_event(mpb_ctx *c)
{
    if (!c->event_pool.empty()) { hipEvent_t e = c->event_pool.back(); c->event_pool.pop_back(); return e; }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
}


void Span::start()
{
    a = get_event(c); b = get_event(c);
    (void)hipEventRecord(a, c->stream);
}

static int resolve_spans(mpb_ctx *c)
{
    if (c->spans.empty()) return MPB_OK;
    HIPCHK(hipStreamSynchronize(c->stream));
    for (auto &s : c->spans) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, s.a, s.b) == hipSuccess) { c->acc_ms[s.kid] += ms; c->acc_n[s.kid] += 1; }
        c->event_pool.push_back(s.a);
        c->event_pool.push_back(s.b);
    }
    c->spans.clear();
    return MPB_OK;
}

int mpb_timing_enable(mpb_ctx *c, int on) { CTXCHK(c); c->timing = on != 0; return MPB_OK; }

int mpb_timing_reset(mpb_ctx *c)
{
    CTXCHK(c);
    int rc = resolve_spans(c);
    if (rc) return rc;
    for (int k = 0; k < MPB_K_COUNT; k++) { c->acc_ms[k] = 0; c->acc_n[k] = 0; }
    return MPB_OK;
}

int mpb_kernel_time(mpb_ctx *c, int kid, double *total_ms, int64_t *launches)
{
    CTXCHK(c);
    if (kid < 0 || kid >= MPB_K_COUNT) return fail(MPB_E_INVALID, "kernel id %d out of range", kid);
    int rc = resolve_spans(c);
    if (rc) return rc;
    if (total_ms) *total_ms = c->acc_ms[kid];
    if (launches) *launches = c->acc_n[kid];
    return MPB_OK;
}
