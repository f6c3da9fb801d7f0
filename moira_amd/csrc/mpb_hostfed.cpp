// mpb_hostfed.cpp -- the host-fed path of the C ABI of libmoira_pb.so (include/moira_pb.h): batches that lie in host memory.
// Small batches take one launch of the one-read-per-wave kernel through pinned memory; everything else the chunked three-stream
// pipeline (H2D | kernels | D2H).  Also: batches with scores above 254 on a private table, and one batch over several GPUs.
// (Every mpb_* and mpbi_* function defined here has C linkage: include/moira_pb.h and mpb_host_internal.h declare them so.)

#include "mpb_ctx.h"

#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>

// Batches of at most MPB_SMALL_N reads (the two paths cost the same at about 8 k reads): one host-to-device copy from pinned memory, one kernel (one read
// per wave), one copy back -- the batched pipeline's eight launches and six copies cost ~150 us whatever
// the size, which is all a per-read caller (bernoulli.calculate_errors_PB) would ever see.
#define MPB_SMALL_N 4096
// small batches whose inputs are at most this many bytes are read by the kernel straight from pinned host memory
// ... and batches of at most this many reads report their completion through a word per read in pinned memory
#define MPB_SMALL_FLAG_N 256
#define MPB_SMALL_ZC_BYTES (1 << 20)

// Wait until done[0..n) all hold `token` (k_small writes it once a read's results are visible to the host).  The kernel
// normally takes tens of microseconds: spin; a launch that has not finished after 20 ms is asked about through the runtime
// (which also reports a fault), and its flags are then looked at once more.
int mpbi_wait_flags(const volatile uint32_t *done, int64_t n, uint32_t token, hipStream_t s)
{
    int64_t k = 0;
    const auto t0 = std::chrono::steady_clock::now();
    for (uint32_t spins = 0;; spins++) {
        while (k < n && done[k] == token) k++;
        if (k == n) { std::atomic_thread_fence(std::memory_order_acquire); return MPB_OK; }
        __builtin_ia32_pause();
        if ((spins & 1023u) == 1023u && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(20)) {
            HIPCHK(hipStreamSynchronize(s));
            while (k < n && done[k] == token) k++;
            if (k == n) return MPB_OK;
            return fail(MPB_E_HIP, "k_small finished without reporting read %lld", (long long)k);
        }
    }
}

static int filter_host_small(mpb_ctx *c, const uint8_t *q, int64_t n, int64_t row_stride, const int32_t *len,
                             int32_t fixed_len, const mpb_filter_params *params, double *ee, int32_t *ns,
                             uint8_t *pass, mpb_filter_counts *counts, bool *done)
{
    *done = false;
    const int32_t max_len = len ? (int32_t)(row_stride < MPB_MAX_LEN ? row_stride : MPB_MAX_LEN) : fixed_len;
    // device staging: inputs | outputs; the pinned block: the same, then a completion word per read
    ChunkArrays d{}, h{};
    uint32_t *h_done = nullptr;
    auto layout = [n, row_stride](Carver &k, ChunkArrays &x) { x.in(k, n, row_stride); x.out(k, n); };
    int rc = carve(c, c->stage, [&](Carver &k) { layout(k, d); });
    if (rc) return rc;
    rc = ensure_workspace(c, n);
    if (rc) return rc;
    c->classified.valid = false;                           // k_small rewrites the class bytes
    if ((rc = carve(c, c->pin_host, [&](Carver &k) { layout(k, h); k.take(h_done, n); }, 2))) return rc;
    const int64_t in_bytes = (char *)d.ee - (char *)d.q, out_bytes = (char *)h_done - (char *)h.ee;
    memcpy(h.q, q, (size_t)(n * row_stride));
    if (len) memcpy(h.len, len, (size_t)(n * 4));
    const MpbDevParams prm = make_dev_params(params, fixed_len, max_len);
    constexpr int64_t zc_bytes = MPB_SMALL_ZC_BYTES;
    if (in_bytes <= zc_bytes) {
        // a handful of reads (the per-read entry: ONE): the kernel reads the rows from, and writes the results to, the pinned
        // host block -- one runtime call instead of three dependent ones (copy in, kernel, copy out) -- and the host learns
        // that the results are there from a word per read in the same block, not from the runtime
        // (a word and a system-scope fence per read pay for a few reads -- 1: 33 -> 27 us, 64: 35 -> 32 -- and cost more than
        // the runtime's one completion signal for many: 1,024 reads 64 -> 82 us; hence the limit)
        const bool flags = n <= MPB_SMALL_FLAG_N;
        if (++c->small_token == 0) c->small_token = 1;
        volatile uint32_t *done = h_done;
        for (int64_t i = 0; flags && i < n; i++) done[i] = 0;
        const MpbSmallHost hostside{d.q, d.ns, flags ? h_done : nullptr, c->small_token};
        { Span t(c, MPB_K_DP); mpb_launch_small(h.q, n, row_stride, len ? h.len : nullptr, prm, c->ws, h.ns, h.ee, h.pass, c->stream, &hostside); }
        HIPCHK(hipGetLastError());
        if (flags) {
            if ((rc = mpbi_wait_flags(done, n, c->small_token, c->stream)) != MPB_OK) return rc;
            if (c->timing) HIPCHK(hipStreamSynchronize(c->stream));      // the spans' events are read after the call
            goto have_results;
        }
    } else {
        HIPCHK(hipMemcpyAsync(d.q, h.q, (size_t)(len ? in_bytes : n * row_stride), hipMemcpyHostToDevice, c->stream));
        { Span t(c, MPB_K_DP); mpb_launch_small(d.q, n, row_stride, len ? d.len : nullptr, prm, c->ws, d.ns, d.ee, d.pass, c->stream); }
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(h.ee, d.ee, (size_t)out_bytes, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(hipStreamSynchronize(c->stream));
have_results:
    const uint8_t *hp = h.pass;
    int64_t np = 0;
    for (int64_t i = 0; i < n; i++) {
        if (hp[i] == 2) return MPB_OK;                     // budget missed: the caller takes the batched path
        np += hp[i];
    }
    memcpy(ee, h.ee, (size_t)(n * 8));
    memcpy(ns, h.ns, (size_t)(n * 4));
    memcpy(pass, hp, (size_t)n);
    if (counts) { counts->n_reads = n; counts->n_pass = np; counts->n_fail = n - np; counts->n_overflow = 0; }
    *done = true;
    return MPB_OK;
}

// ---- host pipeline (SURVEY a-9: chunked batch, async H2D / compute / D2H) ------------------------
//
// Three streams, MPB_HOST_SLOTS (4) chunk slots.  Chunk k (slot k % 4):
//   copy_stream : H2D of its qualities (+ lengths)            -> h2d_done
//   stream      : waits h2d_done, the five kernels of the pass -> k_done
//   out_stream  : waits k_done, D2H of ee / Ns / pass          -> d2h_done
// so that the H2D of chunk k+1 and the D2H of chunk k-1 run beside the kernels of chunk k.  A slot is
// reused only after its previous chunk's d2h_done (which implies its kernels and its H2D are done); a chunk is
// retired three trips after it was queued, AFTER the current trip's work has been queued, so the copy stream
// never runs dry while the host thread copies results out.
// Inputs in pinned host memory (mpb_host_alloc, or registered by the caller) are DMA-ed where they lie;
// pageable inputs are first copied into the slot's pinned staging block by `copy_threads` threads, which
// happens while the GPU is busy with the chunks before.  Outputs always land in the slot's pinned block and
// are copied out when the slot is retired (13 bytes per read).

static bool is_pinned_host(const void *p, size_t bytes)
{
    if (!p || bytes == 0) return false;
    hipPointerAttribute_t a;
    const void *ends[2] = {p, (const char *)p + bytes - 1};
    for (const void *e : ends) {
        memset(&a, 0, sizeof(a));
        if (hipPointerGetAttributes(&a, e) != hipSuccess) { (void)hipGetLastError(); return false; }
        if (a.type != hipMemoryTypeHost) return false;
    }
    return true;
}

void drain_pipeline(mpb_ctx *c)
{
    (void)hipStreamSynchronize(c->copy_stream);
    (void)hipStreamSynchronize(c->stream);
    (void)hipStreamSynchronize(c->out_stream);
    for (auto &sl : c->slot) sl.off = -1;
}

// what a pipeline run computes: the Poisson-binomial pass, or the Poisson approximation (lambda on the device, the
// scalar tail on the host when a chunk is retired -- i.e. beside the GPU work of the chunks after it)
struct PipeJob {
    int poisson;           // 0: Poisson-binomial; 1: lambda + the host tail; 2: lambda + k_poisson_tail (MPB_FLAG_POISSON_DEVICE_TAIL)
    const mpb_filter_params *params;
    const int32_t *len;
    int32_t fixed_len;
    double *ee; int32_t *ns; uint8_t *pass;
    int64_t *n_host_tail;  // poisson == 2: += the reads the host tail finished
};

// wait for the chunk parked in `sl` and hand its results to the caller's arrays
static int retire_slot(mpb_ctx *c, HostSlot &sl, const PipeJob &job, int64_t *n_pass)
{
    if (sl.off < 0) return MPB_OK;
    HIPCHK(hipEventSynchronize(sl.d2h_done));
    const ChunkArrays &h = sl.hout;
    memcpy(job.ns + sl.off, h.ns, (size_t)(sl.m * 4));
    const uint8_t *hp;
    if (job.poisson == 2) {
        // the device tail ran in place: ee / pass as for the Poisson-binomial job, then the host tail on the reads it handed back
        // (pass byte 2, lambda left in the ee slot)
        memcpy(job.ee + sl.off, h.ee, (size_t)(sl.m * 8));
        memcpy(job.pass + sl.off, h.pass, (size_t)sl.m);
        int64_t marked = 0;
        int rc = poisson_finish_marked(job.params, job.ns + sl.off, job.len ? job.len + sl.off : nullptr, job.fixed_len, sl.m,
                                       job.ee + sl.off, job.pass + sl.off, &marked);
        if (rc) return rc;
        *job.n_host_tail += marked;
        hp = job.pass + sl.off;
    } else if (job.poisson) {
        // the block's first array holds lambda; ee / pass come from the reference's scalar loop (moira.py:1666-1679)
        int rc = mpb_poisson_finish_host(h.ee, job.ns + sl.off, job.len ? job.len + sl.off : nullptr, job.fixed_len,
                                         sl.m, job.params, job.ee + sl.off, job.pass + sl.off);
        if (rc) return rc;
        hp = job.pass + sl.off;
    } else {
        memcpy(job.ee + sl.off, h.ee, (size_t)(sl.m * 8));
        hp = h.pass;
        memcpy(job.pass + sl.off, hp, (size_t)sl.m);
    }
    int64_t np = 0;
    for (int64_t i = 0; i < sl.m; i++) np += hp[i];
    *n_pass += np;
    sl.off = -1;
    return MPB_OK;
}

int filter_host_pipeline(mpb_ctx *c, const uint8_t *q, int64_t n, int64_t row_stride, const int32_t *len,
                         int32_t fixed_len, const mpb_filter_params *params, double *ee, int32_t *ns,
                         uint8_t *pass, mpb_filter_counts *counts, int poisson)
{
    int64_t n_host_tail = 0;
    const PipeJob job = {poisson, params, len, fixed_len, ee, ns, pass, &n_host_tail};
    const MpbDevParams tail_prm = make_dev_params(params, fixed_len, 1);         // poisson == 2: what k_poisson_tail reads
    const int64_t chunk = pipeline_chunk_reads(n, row_stride);
    const bool q_pinned = is_pinned_host(q, (size_t)(n * row_stride));
    const bool len_pinned = len && is_pinned_host(len, (size_t)(n * 4));
    const int64_t nchunks = (n + chunk - 1) / chunk;
    const int nslots = (int)(nchunks < MPB_HOST_SLOTS ? nchunks : MPB_HOST_SLOTS);
    int rc = ensure_workspace(c, chunk);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));
    for (int k = 0; k < nslots; k++) {                       // the slots' blocks, laid out for chunks of this call's size
        HostSlot &sl = c->slot[k];
        sl.off = -1;
        if ((rc = carve(c, sl.dev, [&](Carver &cv) { sl.d.in(cv, chunk, row_stride); sl.d.out(cv, chunk); }))) return rc;
        if ((rc = carve(c, sl.pin_out, [&](Carver &cv) { sl.hout.out(cv, chunk); }))) return rc;
        if (!(q_pinned && (!len || len_pinned)))
            if ((rc = carve(c, sl.pin_in, [&](Carver &cv) { sl.hin.in(cv, chunk, row_stride); }))) return rc;
    }
    HIPCHK(hipMemsetAsync(c->ws.ovf_total, 0, sizeof(long long), c->stream));
    // the host has validated every length: a count left behind by an earlier mpb_filter_device call that never
    // fetched its counts must not fail this one
    HIPCHK(hipMemsetAsync(c->ws.bad_len, 0, sizeof(int32_t), c->stream));
    if (poisson) HIPCHK(hipMemsetAsync(c->ws.ovf_count, 0, sizeof(int32_t), c->stream));     // reads with a byte 255, summed over the chunks
    if (poisson == 2) {    // the device tail's counters (neither is fetched here: the host sees every pass byte anyway)
        HIPCHK(hipMemsetAsync(c->ws.pt_count, 0, sizeof(int32_t), c->stream));
        HIPCHK(hipMemsetAsync(c->ws.pass_count, 0, sizeof(unsigned long long), c->stream));
    }
    int64_t n_pass = 0;
    int64_t k = 0;
    for (int64_t off = 0; off < n; off += chunk, k++) {
        const int64_t m = (n - off < chunk) ? n - off : chunk;
        HostSlot &sl = c->slot[k % MPB_HOST_SLOTS];          // free: its previous chunk (k - 4) was retired in trip k - 1
        uint8_t *d_q = sl.d.q, *d_pass = sl.d.pass;
        int32_t *d_len = sl.d.len, *d_ns = sl.d.ns;
        double *d_ee = sl.d.ee;
        // ---- H2D ----
        const uint8_t *src_q = q + off * row_stride;
        if (!q_pinned) {
            parallel_copy(sl.hin.q, src_q, (size_t)(m * row_stride), c->copy_threads);
            src_q = sl.hin.q;
        }
        hipError_t e = hipMemcpyAsync(d_q, src_q, (size_t)(m * row_stride), hipMemcpyHostToDevice, c->copy_stream);
        if (e == hipSuccess && len) {
            const int32_t *src_len = len + off;
            if (!len_pinned) {
                memcpy(sl.hin.len, src_len, (size_t)(m * 4));
                src_len = sl.hin.len;
            }
            e = hipMemcpyAsync(d_len, src_len, (size_t)(m * 4), hipMemcpyHostToDevice, c->copy_stream);
        }
        if (e == hipSuccess) e = hipEventRecord(sl.h2d_done, c->copy_stream);
        // ---- kernels ----
        if (e == hipSuccess) e = hipStreamWaitEvent(c->stream, sl.h2d_done, 0);
        if (e != hipSuccess) { drain_pipeline(c); return fail(MPB_E_HIP, "host pipeline (H2D): %s", hipGetErrorString(e)); }
        if (poisson) {
            Span t(c, MPB_K_LAMBDA);
            mpb_launch_lambda(d_q, m, row_stride, len ? d_len : nullptr, fixed_len, c->ws.lut, d_ee, d_ns, c->ws.ovf_count, c->stream);
            rc = hipGetLastError() == hipSuccess ? MPB_OK : fail(MPB_E_HIP, "k_lambda launch failed");
        }
        if (poisson == 2 && rc == MPB_OK) {
            Span t(c, MPB_K_POISSON_TAIL);           // in place: lambda sits in the chunk's ee array
            mpb_launch_poisson_tail(d_ee, d_ns, len ? d_len : nullptr, m, tail_prm, d_ee, d_pass, c->ws.pt_count, nullptr, 0,
                                    c->ws.pass_count, c->stream);
            rc = hipGetLastError() == hipSuccess ? MPB_OK : fail(MPB_E_HIP, "k_poisson_tail launch failed");
        }
        if (!poisson) {
            // (the chunks always take the sorted pipeline: the narrow pass synchronises on its count of handed-back reads, which would
            // stall the three-stream overlap of a path that is bound by the link anyway)
            mpb_filter_params chunk_prm = *params;
            chunk_prm.flags = (chunk_prm.flags & ~((15u << 8) | (255u << 12))) | MPB_FLAG_NO_NARROW;
            rc = mpb_filter_device(c, d_q, m, row_stride, len ? d_len : nullptr, fixed_len, &chunk_prm, d_ee, d_ns, d_pass, nullptr);
        }
        if (rc) { drain_pipeline(c); return rc; }
        e = hipEventRecord(sl.k_done, c->stream);
        // ---- D2H ----
        if (e == hipSuccess) e = hipStreamWaitEvent(c->out_stream, sl.k_done, 0);
        if (e == hipSuccess) e = hipMemcpyAsync(sl.hout.ee, d_ee, (size_t)((char *)d_pass - (char *)d_ee + align_up(m, 256)),
                                                hipMemcpyDeviceToHost, c->out_stream);
        if (e == hipSuccess) e = hipEventRecord(sl.d2h_done, c->out_stream);
        if (e != hipSuccess) { drain_pipeline(c); return fail(MPB_E_HIP, "host pipeline (D2H): %s", hipGetErrorString(e)); }
        sl.off = off; sl.m = m;
        // With this chunk queued behind the two before it, hand chunk k - 3 to the caller: the host-side copy
        // of its results (and, next trip, the staging copy of chunk k + 1) runs while the copy engines are busy
        // with queued work, and frees the slot the next trip fills.
        if ((rc = retire_slot(c, c->slot[(k + 1) % MPB_HOST_SLOTS], job, &n_pass))) { drain_pipeline(c); return rc; }
        // ... and any younger chunk whose results have already landed (in order), so that little is left for the end
        for (int64_t j = k + 2; j <= k + MPB_HOST_SLOTS - 1; j++) {
            HostSlot &o = c->slot[j % MPB_HOST_SLOTS];
            if (o.off < 0) continue;
            if (hipEventQuery(o.d2h_done) != hipSuccess) { (void)hipGetLastError(); break; }
            if ((rc = retire_slot(c, o, job, &n_pass))) { drain_pipeline(c); return rc; }
        }
    }
    // retire what is still in flight, oldest first
    for (int64_t j = k; j < k + MPB_HOST_SLOTS; j++)
        if ((rc = retire_slot(c, c->slot[j % MPB_HOST_SLOTS], job, &n_pass))) { drain_pipeline(c); return rc; }
    PinWords &w = *c->pin;                           // (pinned: an early return leaves no copy in flight into a dead frame)
    w.ovf_total = 0;
    w.bad_len = w.bad255 = 0;
    HIPCHK(hipMemcpyAsync(&w.ovf_total, c->ws.ovf_total, sizeof(w.ovf_total), hipMemcpyDeviceToHost, c->stream));
    if (len && !poisson) HIPCHK(hipMemcpyAsync(&w.bad_len, c->ws.bad_len, sizeof(w.bad_len), hipMemcpyDeviceToHost, c->stream));
    if (poisson) HIPCHK(hipMemcpyAsync(&w.bad255, c->ws.ovf_count, sizeof(w.bad255), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    const int32_t bad = w.bad_len, bad255 = w.bad255;
    long long ovf = w.ovf_total;
    if (bad255) return fail(MPB_E_INVALID, "%d read(s) contain byte 255 ('n'): the Poisson path follows the Python reference, "
                            "which scores lower-case n as a normal base -- pack it as one", bad255);
    if (poisson) ovf = n_host_tail;                  // (0 without MPB_FLAG_POISSON_DEVICE_TAIL)
    if (bad) {
        HIPCHK(hipMemsetAsync(c->ws.bad_len, 0, sizeof(int32_t), c->stream));
        return fail(MPB_E_INVALID, "%d read length(s) outside 0..%d", bad, MPB_MAX_LEN);
    }
    if (counts) { counts->n_reads = n; counts->n_pass = n_pass; counts->n_fail = n - n_pass; counts->n_overflow = ovf; }
    return MPB_OK;
}

int mpb_filter_host(mpb_ctx *c, const uint8_t *q, int64_t n, int64_t row_stride, const int32_t *len,
                    int32_t fixed_len, const mpb_filter_params *params, double *ee, int32_t *ns,
                    uint8_t *pass, mpb_filter_counts *counts)
{
    CTXCHK(c);
    int rc = check_params(params);
    if (rc) return rc;
    if (n < 0) return fail(MPB_E_INVALID, "n < 0");
    if (row_stride <= 0 || row_stride % 16 != 0) return fail(MPB_E_INVALID, "row_stride must be a positive multiple of 16");
    if (row_stride > MPB_MAX_STRIDE) return fail(MPB_E_INVALID, "row_stride %lld exceeds %d (reads longer than %d bases are not supported)", (long long)row_stride, MPB_MAX_STRIDE, MPB_MAX_LEN);
    if (n > 0 && (!q || !ee || !ns || !pass)) return fail(MPB_E_INVALID, "NULL host buffer");
    if (!len && (fixed_len < 0 || fixed_len > row_stride)) return fail(MPB_E_INVALID, "fixed_len %d does not fit row_stride %lld", fixed_len, (long long)row_stride);
    if (!len && fixed_len > MPB_MAX_LEN) return fail(MPB_E_INVALID, "reads longer than %d bases are not supported", MPB_MAX_LEN);
    if (len) {
        // a length is never clamped silently: the reference scores every base it is given
        const int64_t lim = row_stride < MPB_MAX_LEN ? row_stride : MPB_MAX_LEN;
        for (int64_t i = 0; i < n; i++)
            if (len[i] < 0 || len[i] > lim)
                return fail(MPB_E_INVALID, len[i] > row_stride || len[i] < 0 ? "read %lld: length %d does not fit the %lld-byte row"
                                                                             : "read %lld: %d bases; reads longer than 65535 bases are not supported (row of %lld bytes)",
                            (long long)i, len[i], (long long)row_stride);
    }
    if (counts) { counts->n_reads = n; counts->n_pass = 0; counts->n_fail = 0; counts->n_overflow = 0; }
    if (n == 0) return MPB_OK;
    if (n <= MPB_SMALL_N && n * row_stride <= (8ll << 20) && row_stride <= MPB_SMALL_MAX_STRIDE && !(params->flags & MPB_FLAG_BATCHED_ONLY)) {
        bool done = false;
        rc = filter_host_small(c, q, n, row_stride, len, fixed_len, params, ee, ns, pass, counts, &done);
        if (rc || done) return rc;
    }
    return filter_host_pipeline(c, q, n, row_stride, len, fixed_len, params, ee, ns, pass, counts, 0);
}

int mpb_filter_host_coded(mpb_ctx *c, const uint8_t *q, int64_t n, int64_t row_stride, const int32_t *len, int32_t fixed_len,
                          const mpb_filter_params *params, const int32_t *code_scores, double *ee, int32_t *ns, uint8_t *pass,
                          mpb_filter_counts *counts)
{
    CTXCHK(c);
    if (!code_scores) return mpb_filter_host(c, q, n, row_stride, len, fixed_len, params, ee, ns, pass, counts);
    MpbPair h[256];
    build_lut(h);
    bool any = false;
    for (int code = 1; code <= 254; code++) {
        if (code_scores[code] == code) continue;
        if (code_scores[code] < 1) return fail(MPB_E_RANGE, "code %d stands for score %d: scores are >= 1 (Q0 is clamped to 1 at pack time)", code, code_scores[code]);
        lut_entry(code_scores[code], &h[code]);
        any = true;
    }
    PrivateTable guard(c);
    int rc;
    if (any && (rc = guard.install((const double2 *)h)) != MPB_OK) return rc;
    return mpb_filter_host(c, q, n, row_stride, len, fixed_len, params, ee, ns, pass, counts);
}

// ---- one host process, several GPUs ("one host thread (or process) + one HIP stream per device") ----
//
// The batch is cut into n_ctx contiguous, balanced shards in read order (shard r = reads [r*n/W + min(r, n%W), ...), the
// same bounds as moira_amd/shard.py:shard_bounds); one host thread per context runs the ordinary host pipeline on its
// shard and writes straight into the caller's arrays at the shard's offset, so the results come back gathered in read
// order with no copy and no exchange step.  Every context keeps its own streams, slots and workspace (contexts are
// independent: tests/test_gpu_parity.py::test_two_contexts_from_two_threads); a host-fed caller thereby drives one
// PCIe link per GPU from one process -- what moira's `Pool(args.processors)` (moira/moira.py:398-399) was for.
// ---- NUMA placement of a shard's host thread (8 x 55 GB/s out of one socket does not scale) ------------------
// The PCI device of a GPU says which NUMA node it hangs off (/sys/bus/pci/devices/<id>/numa_node) and the node says which CPUs
// are its own (/sys/devices/system/node/node<k>/cpulist).  A shard thread of mpb_filter_host_multi restricts itself to those
// CPUs before it starts its pipeline: the pinned staging blocks of its slots are then allocated and first touched from that
// node, and the threads that copy a pageable input into them inherit the mask.  `sysfs_root` ("" = the real one) exists for
// the parser's test.  node -1 (no NUMA information, one node, a container that hides it) leaves the thread where it is.
// restrict the calling thread to the CPUs of `c`'s GPU's NUMA node that this process may use; returns the node or -1 (not moved)
static int pin_thread_near_device(const mpb_ctx *c)
{
    if (getenv("MOIRA_PB_NO_NUMA")) return -1;
    char bus[64] = "";
    if (hipDeviceGetPCIBusId(bus, (int)sizeof(bus), c->device) != hipSuccess) return -1;
    int32_t node = -1;
    char list[4096];
    if (mpb_numa_cpulist_for_pci("", bus, &node, list, (int32_t)sizeof(list)) != MPB_OK || node < 0) return -1;
    cpu_set_t near, allowed, both;
    if (!parse_cpulist(list, &near, nullptr)) return -1;
    if (sched_getaffinity(0, sizeof(allowed), &allowed) != 0) return -1;
    CPU_AND(&both, &near, &allowed);
    if (CPU_COUNT(&both) == 0) return -1;                                    // the cgroup grants nothing on that node: stay
    if (sched_setaffinity(0, sizeof(both), &both) != 0) return -1;
    return node;
}

int mpb_filter_host_multi(mpb_ctx *const *ctxs, int32_t n_ctx, const uint8_t *q, int64_t n, int64_t row_stride,
                          const int32_t *len, int32_t fixed_len, const mpb_filter_params *params, double *ee,
                          int32_t *ns, uint8_t *pass, mpb_filter_counts *counts, int32_t poisson)
{
    if (!ctxs || n_ctx < 1) return fail(MPB_E_INVALID, "mpb_filter_host_multi: no context");
    for (int k = 0; k < n_ctx; k++) {
        if (!ctxs[k]) return fail(MPB_E_INVALID, "mpb_filter_host_multi: context %d is NULL", k);
        for (int j = 0; j < k; j++)
            if (ctxs[j] == ctxs[k]) return fail(MPB_E_INVALID, "mpb_filter_host_multi: context %d is listed twice (calls on one context must not overlap)", k);
    }
    if (n < 0) return fail(MPB_E_INVALID, "n < 0");
    if (counts) { counts->n_reads = n; counts->n_pass = 0; counts->n_fail = 0; counts->n_overflow = 0; }
    struct Shard { int64_t lo = 0, hi = 0; int rc = MPB_OK; mpb_filter_counts c{}; char err[MPB_ERR_LEN] = ""; };
    std::vector<Shard> sh((size_t)n_ctx);
    for (int r = 0; r < n_ctx; r++) (void)mpb_shard_bounds(n, n_ctx, r, &sh[(size_t)r].lo, &sh[(size_t)r].hi);
    auto work = [&](int r) {
        Shard &S = sh[(size_t)r];
        const int64_t m = S.hi - S.lo;
        // the shard's thread (and the copy threads it starts, and the pinned blocks it first touches) next to its GPU; the
        // calling thread (shard 0, and shards that got no thread) gets its own mask back afterwards
        cpu_set_t before;
        const bool have_before = n_ctx > 1 && sched_getaffinity(0, sizeof(before), &before) == 0;
        if (n_ctx > 1) (void)pin_thread_near_device(ctxs[r]);
        const uint8_t *qs = q ? q + S.lo * row_stride : q;
        const int32_t *ls = len ? len + S.lo : nullptr;
        if (poisson)
            S.rc = mpb_filter_poisson_host(ctxs[r], qs, m, row_stride, ls, fixed_len, params, ee ? ee + S.lo : ee,
                                           ns ? ns + S.lo : ns, pass ? pass + S.lo : pass, &S.c);
        else
            S.rc = mpb_filter_host(ctxs[r], qs, m, row_stride, ls, fixed_len, params, ee ? ee + S.lo : ee,
                                   ns ? ns + S.lo : ns, pass ? pass + S.lo : pass, &S.c);
        if (S.rc != MPB_OK) snprintf(S.err, sizeof(S.err), "%s", mpb_last_error());      // the error text is thread-local: carry it out
        if (have_before) (void)sched_setaffinity(0, sizeof(before), &before);
    };
    std::vector<std::thread> th;
    int started = 1;                                   // shard 0 runs on the calling thread
    try {
        th.reserve((size_t)n_ctx);
        for (int r = 1; r < n_ctx; r++) { th.emplace_back(work, r); started = r + 1; }
    } catch (...) {
        // no thread to be had: the shards that got none run on this thread, one after the other
    }
    work(0);
    for (int r = started; r < n_ctx; r++) work(r);
    for (auto &t : th) t.join();
    for (int r = 0; r < n_ctx; r++) {
        const Shard &S = sh[(size_t)r];
        if (S.rc != MPB_OK) return fail(S.rc, "shard %d of %d (reads %lld..%lld): %s", r, n_ctx, (long long)S.lo, (long long)S.hi - 1, S.err);
        if (counts) { counts->n_pass += S.c.n_pass; counts->n_fail += S.c.n_fail; counts->n_overflow += S.c.n_overflow; }
    }
    return MPB_OK;
}
