// StreamQueue (moira_amd/csrc/mpb_queue.h) without a device: this file is the header's second includer.  It provides the names the
// header is written against -- a runtime that records every call and can be told to fail chosen calls -- and drives the queue
// through a fixed script, once with no failure and once per failing call, and through the scopes that matter to its destructor.
// tests/test_stream_queue_model.py builds it with the address and undefined-behaviour sanitizers and runs it as a program; built
// with -DSTREAM_QUEUE_NO_DTOR_SYNC (the destructor does nothing) the destructor checks, and only they, must fail.
//
// The log holds one letter per call: U / D hipMemcpyAsync up / down, Z hipMemsetAsync, ( and ) a Span opened and closed, L a
// launch inside it, G hipGetLastError, Y hipStreamSynchronize.  The calls that can fail (U D Z G Y) are numbered as they come.
// Prints "script: <n> checks, <f> failed" and "destructor: <n> checks, <f> failed"; exit status 1 when anything failed.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

#include "moira_pb.h"                            // MPB_OK, MPB_E_HIP, MPB_E_NOMEM

// ---- the stub: what mpb_ctx.h provides inside the library ------------------------------------------------------------------------
typedef int hipError_t;
enum { hipSuccess = 0, hipErrorOutOfMemory = 2, hipErrorLaunchFailure = 719, hipErrorUnknown = 999 };
enum hipMemcpyKind { hipMemcpyHostToDevice = 1, hipMemcpyDeviceToHost = 2 };
typedef int *hipStream_t;
struct mpb_ctx { hipStream_t stream; };

static std::string g_log, g_what;
static int g_calls = 0, g_foreign = 0;           // failable calls so far; calls on a stream that is not the context's
static hipError_t g_fail[32];                    // g_fail[k]: what the k-th failable call returns
static int g_stream_word;

static hipError_t record(char what, hipStream_t s)
{
    g_log += what;
    if (s != &g_stream_word) g_foreign++;
    return g_calls < 32 ? g_fail[g_calls++] : hipSuccess;
}
static hipError_t hipMemcpyAsync(void *, const void *, size_t, hipMemcpyKind k, hipStream_t s) { return record(k == hipMemcpyHostToDevice ? 'U' : 'D', s); }
static hipError_t hipMemsetAsync(void *, int, size_t, hipStream_t s) { return record('Z', s); }
static hipError_t hipGetLastError() { return record('G', &g_stream_word); }
static hipError_t hipStreamSynchronize(hipStream_t s) { return record('Y', s); }
struct Span {
    Span(mpb_ctx *, int kid) { g_log += kid == 7 ? '(' : '?'; }
    ~Span() { g_log += ')'; }
};
static int hip_fail(const char *what, hipError_t e)
{
    g_what = what;
    return e == hipErrorOutOfMemory ? MPB_E_NOMEM : MPB_E_HIP;
}

#include "mpb_queue.h"

// ---- the checks ------------------------------------------------------------------------------------------------------------------
static int g_checks = 0, g_failed = 0;
static const char *g_section = "script";
static void check(bool ok, const char *what, int k, int k2)
{
    g_checks++;
    if (ok) return;
    g_failed++;
    std::printf("FAIL %s: %s (failing calls %d, %d; log %s)\n", g_section, what, k, k2, g_log.c_str());
}
static void reset(int k, hipError_t e, int k2 = -1, hipError_t e2 = hipSuccess)
{
    g_log.clear(); g_what.clear(); g_calls = 0; g_foreign = 0;
    memset(g_fail, 0, sizeof(g_fail));
    if (k >= 0) g_fail[k] = e;
    if (k2 >= 0) g_fail[k2] = e2;
}
static int code_of(hipError_t e) { return e == hipSuccess ? MPB_OK : e == hipErrorOutOfMemory ? MPB_E_NOMEM : MPB_E_HIP; }

// up, up, zero, run with two launches inside, down, down, wait, up, wait -- with zero-byte calls strewn in, which record nothing.
// The failable calls, in order: 0 U, 1 U, 2 Z, 3 G, 4 D, 5 D, 6 Y, 7 U, 8 Y.
static const char *const k_ops[9] = {"U", "U", "Z", "(LL)G", "D", "D", "Y", "U", "Y"};
static void script(int k, hipError_t e, int k2 = -1, hipError_t e2 = hipSuccess)
{
    reset(k, e, k2, e2);
    mpb_ctx c{&g_stream_word};
    char host[64], dev[64];
    int rc1, rc2;
    std::string what1, what2;
    {
        StreamQueue q(&c);
        q.up(dev, host, 0);
        q.up(dev, host, 16);
        q.up(dev + 16, host + 16, 8);
        q.zero(dev, 0);
        q.zero(dev + 32, 32);
        q.run(7, [&] { g_log += 'L'; g_log += 'L'; });
        q.down(host, dev, 16);
        q.down(host, dev, 0);
        q.down(host + 16, dev + 16, 8);
        rc1 = q.wait("first");
        what1 = g_what;
        g_what.clear();
        q.up(dev, host, 16);
        q.down(host, dev, 0);
        rc2 = q.wait("second");
        what2 = g_what;
    }
    // the model: nothing is recorded behind a failing call but the one synchronisation, which also makes the queue usable again.
    // k and k2 count the failable calls that are MADE, so behind a failure the synchronisation is the next one.
    std::string want, want_what[2];
    hipError_t kept = hipSuccess;
    int want_rc[2] = {MPB_OK, MPB_OK}, made = 0;
    for (int i = 0, w = 0; i < 9; i++) {
        const bool is_wait = k_ops[i][0] == 'Y';
        if (!is_wait && kept != hipSuccess) continue;
        want += k_ops[i];
        const hipError_t got = made == k ? e : made == k2 ? e2 : hipSuccess;
        made++;
        if (!is_wait) { kept = got; continue; }
        // a kept failure is reported as `what`, a synchronisation's own as itself -- and only when nothing was kept
        want_rc[w] = code_of(kept != hipSuccess ? kept : got);
        want_what[w] = kept != hipSuccess ? (w ? "second" : "first") : got != hipSuccess ? "hipStreamSynchronize" : "";
        kept = hipSuccess;
        w++;
    }
    check(g_log == want, ("the recorded calls are not " + want).c_str(), k, k2);
    check(g_foreign == 0, "a call went to another stream", k, k2);
    int syncs = 0;
    for (char ch : g_log) syncs += ch == 'Y';
    check(syncs == 2, "each wait synchronises exactly once, and the destructor not at all", k, k2);
    check(rc1 == want_rc[0] && rc2 == want_rc[1], "a wait's code is not that of the first failure since the wait before", k, k2);
    check(what1 == want_what[0] && what2 == want_what[1], "a wait names the wrong call", k, k2);
}

static void destructor()
{
    g_section = "destructor";
    mpb_ctx c{&g_stream_word};
    char host[16], dev[16];
    reset(-1, hipSuccess);
    { StreamQueue q(&c); q.up(dev, host, 16); }
    check(g_log == "UY", "a pending copy is not waited for when the scope is left", -1, -1);
    reset(-1, hipSuccess);
    { StreamQueue q(&c); q.run(7, [] {}); }
    check(g_log == "()GY", "a pending launch is not waited for when the scope is left", -1, -1);
    reset(1, hipErrorLaunchFailure);
    { StreamQueue q(&c); q.down(host, dev, 16); q.zero(dev, 16); q.up(dev, host, 16); }
    check(g_log == "DZY", "a pending copy with a kept failure is not waited for when the scope is left", 1, -1);
    reset(0, hipErrorOutOfMemory);
    { StreamQueue q(&c); q.up(dev, host, 16); q.down(host, dev, 16); }
    check(g_log == "UY", "a kept failure alone is not waited for when the scope is left", 0, -1);
    reset(-1, hipSuccess);
    { StreamQueue q(&c); q.up(dev, host, 16); (void)q.wait("w"); }
    check(g_log == "UY", "the destructor synchronises again after a wait", -1, -1);
    reset(0, hipErrorUnknown);
    { StreamQueue q(&c); q.up(dev, host, 16); (void)q.wait("w"); }
    check(g_log == "UY", "the destructor synchronises again after a wait that reported a failure", 0, -1);
    reset(-1, hipSuccess);
    { StreamQueue q(&c); }
    check(g_log.empty(), "the destructor synchronises when nothing was queued", -1, -1);
    reset(-1, hipSuccess);
    { StreamQueue q(&c); q.up(dev, host, 0); q.down(host, dev, 0); q.zero(dev, 0); }
    check(g_log.empty(), "zero-byte calls are recorded or waited for", -1, -1);
    reset(-1, hipSuccess);
    { StreamQueue q(&c); q.up(dev, host, 16); (void)q.wait("w"); q.down(host, dev, 16); }
    check(g_log == "UYDY", "a copy queued behind a wait is not waited for when the scope is left", -1, -1);
}

int main()
{
    const hipError_t errs[3] = {hipErrorOutOfMemory, hipErrorLaunchFailure, hipErrorUnknown};
    script(-1, hipSuccess);
    for (int k = 0; k < 9; k++)
        for (hipError_t e : errs) script(k, e);
    // two failures in one run: behind failing call k < 6 the synchronisation is call k + 1 (its failure is not reported: the kept
    // one is, whichever of the two is out-of-memory), the second part's copy k + 2 and its synchronisation k + 3
    for (int k = 0; k < 9; k++)
        for (int k2 = k + 1; k2 < 9 && k2 <= k + 3; k2++) {
            script(k, hipErrorOutOfMemory, k2, hipErrorLaunchFailure);
            script(k, hipErrorLaunchFailure, k2, hipErrorOutOfMemory);
        }
    std::printf("script: %d checks, %d failed\n", g_checks, g_failed);
    const int checks0 = g_checks, failed0 = g_failed;
    destructor();
    std::printf("destructor: %d checks, %d failed\n", g_checks - checks0, g_failed - failed0);
    return g_failed != 0;
}
