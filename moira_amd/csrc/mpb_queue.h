// mpb_queue.h -- StreamQueue: the calls one staged host entry queues on its context's stream (uploads, memsets, launches,
// read-backs), the one wait for them, and the invariant the staged entries share: nothing returns while a copy into or out of a
// frame, a vector or the caller's array is in flight.  The queue keeps the first call that failed and queues nothing after it;
// wait() always synchronises, whatever was kept; a queue that leaves its scope with something queued since the last wait()
// synchronises in its destructor, so every early return between a queued copy and its wait is safe.  Declare it AFTER the host
// blocks it copies from and into (it must leave first).
// Includes no HIP header: it is written against names its includer provides (hipError_t, hipSuccess, hipStream_t, hipMemcpyKind
// and its two directions, hipMemcpyAsync, hipMemsetAsync, hipGetLastError, hipStreamSynchronize, Span, hip_fail, MPB_OK and an
// mpb_ctx with a `stream`).  In the library that is mpb_ctx.h; tests/helpers/stream_queue_check.cpp is the other includer, with
// a runtime that records every call.  (run() takes any callable, as carve() takes any layout; nothing else is a template.)
#ifndef MPB_QUEUE_H
#define MPB_QUEUE_H

struct StreamQueue {
    mpb_ctx *c;
    hipError_t kept = hipSuccess;                        // the first call that failed since the last wait()
    bool pending = false;                                // something was queued (or tried) since the last wait()
    explicit StreamQueue(mpb_ctx *ctx) : c(ctx) {}
    StreamQueue(const StreamQueue &) = delete;
    StreamQueue &operator=(const StreamQueue &) = delete;
    ~StreamQueue()
    {
#ifndef STREAM_QUEUE_NO_DTOR_SYNC                        // (the checker's sensitivity build)
        if (pending) (void)hipStreamSynchronize(c->stream);
#endif
    }
    bool ok() const { return kept == hipSuccess; }
    void up(void *dst, const void *src, int64_t bytes) { copy(dst, src, bytes, hipMemcpyHostToDevice); }
    void down(void *dst, const void *src, int64_t bytes) { copy(dst, src, bytes, hipMemcpyDeviceToHost); }
    void zero(void *dst, int64_t bytes)
    {
        if (bytes > 0 && ok()) { pending = true; kept = hipMemsetAsync(dst, 0, (size_t)bytes, c->stream); }
    }
    void ones(void *dst, int64_t bytes)                  // every byte 0xFF
    {
        if (bytes > 0 && ok()) { pending = true; kept = hipMemsetAsync(dst, 0xFF, (size_t)bytes, c->stream); }
    }
    // the launches of fn() (one launch wrapper or several) inside one timing span of kernel id `kid`
    template <typename Fn> void run(int kid, Fn &&fn)
    {
        if (!ok()) return;
        pending = true;
        { Span t(c, kid); fn(); }
        kept = hipGetLastError();
    }
    // the one synchronisation: the kept failure (as `what`), else the synchronisation's own, else MPB_OK; the queue is empty after it
    int wait(const char *what)
    {
        const hipError_t e = kept, e_sync = hipStreamSynchronize(c->stream);
        kept = hipSuccess;
        pending = false;
        if (e != hipSuccess) return hip_fail(what, e);
        if (e_sync != hipSuccess) return hip_fail("hipStreamSynchronize", e_sync);
        return MPB_OK;
    }

private:
    void copy(void *dst, const void *src, int64_t bytes, hipMemcpyKind kind)
    {
        if (bytes > 0 && ok()) { pending = true; kept = hipMemcpyAsync(dst, src, (size_t)bytes, kind, c->stream); }
    }
};

#endif
