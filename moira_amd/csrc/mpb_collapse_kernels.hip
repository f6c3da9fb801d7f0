// mpb_collapse_kernels.hip -- the data-parallel part of the collapse of identical sequences on the device (include/moira_pb.h,
// mpb_collapse_text_host): for records k < n of a text and its record index, the CPython-2.7 string hash of the (truncated)
// sequence -- the value py2_hash gives (csrc/fastio.cpp) -- and rep[k], the first record of the chunk with the same sequence.
// mio_collapse_add_grouped takes both; the host's group table stays the owner of everything that crosses chunks.
//   k_col_hash   one lane per record: the row by its check (it is not trusted, uploaded or device-written), hash[k]; the first k
//                whose row fails by an atomic min into status[0].  The recurrence has no parallel form, so a record's chain is
//                one lane's; the text comes in whole aligned 16-byte words, each fetched once.
//   k_col_group  one lane per record: linear probing over `cap` owner slots (a power of two >= 2 n, all empty at launch) from a
//                slot derived from hash[k], one atomic compare-and-swap of empty -> k per slot; the record stays where it wins
//                or where the owner has its hash, its length AND its bytes; then an atomic min of k into first[slot].
//   k_col_rep    rep[k] = first[slot of k], an int32: the smallest k' <= k with an equal sequence, whoever owned the slot.
// THE RULE OF THE UNIT: inside k_col_group the lanes talk to each other only through the return values of its two atomics.
// Every other byte a lane reads there -- the text, the index, hash[] -- was written before the launch, and what the launch
// writes (the table, first[], slot[]) is read by plain loads only in the NEXT launch.  That is why no fence protocol is needed
// between workgroups on different XCDs.  No lane waits for another lane's progress; every loop is bounded by a checked length
// or by cap.
// One lane per record in k_col_group too, not a lane group as the formatter's FM_GROUP: the compare runs once for a record that
// meets its own sequence (an equal 64-bit hash and length in front of it), reads what k_col_hash read without that kernel's
// dependent chain, and the lanes of a wave stand at different slots of different probe walks, so a group would buy shuffles in
// a loop that is divergent by nature; it also keeps the lane code free of wave intrinsics for the host model.
// What a lane does is mpb_collapse_lane.inc (also compiled and checked on the host).  All results leave by plain vector stores
// and vector atomics.  The kernels have no timing id of their own (the table of MPB_K_* ids is pinned at 22): the host queues
// them inside MPB_K_PACK_TEXT's span, as the formatter's.

#include "mpb_internal.h"

#define CL_FN __device__ __forceinline__
#define CL_LD_I64(p, k) ((p)[k])
#define CL_LD_U64(p, k) ((p)[k])
#define CL_LD_U32(p, k) ((p)[k])
#define CL_LD_SLOT(p, k) ((p)[k])
#define CL_LD16(text, off) cl_gload16((text) + (off))
#define CL_ST_U64(p, k, v) ((p)[k] = (v))
#define CL_ST_I32(p, k, v) ((p)[k] = (v))
#define CL_ST_SLOT(p, k, v) ((p)[k] = (v))
#define CL_CAS_I32(p, s, want, v) cl_cas((p) + (s), (want), (v))
#define CL_MIN_U32(p, s, v) ((void)__hip_atomic_fetch_min((p) + (s), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
struct cl_w16;
__device__ __forceinline__ cl_w16 cl_gload16(const uint8_t *p);
__device__ __forceinline__ int32_t cl_cas(int32_t *p, int32_t want, int32_t v)
{
    (void)__hip_atomic_compare_exchange_strong(p, &want, v, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return want;                                             // (what the slot held: `want` itself when the swap took place)
}
#include "mpb_collapse_lane.inc"
__device__ __forceinline__ cl_w16 cl_gload16(const uint8_t *p)
{
    const uint4 v = *reinterpret_cast<const uint4 *>(p);
    cl_w16 o;
    o.w[0] = v.x; o.w[1] = v.y; o.w[2] = v.z; o.w[3] = v.w;
    return o;
}

static_assert(CL_LANES == 256 && sizeof(ClParams) <= 64, "the collapse kernels' shapes");

namespace {

__global__ __launch_bounds__(CL_LANES) void k_col_hash(const uint8_t *__restrict__ text, const int64_t *__restrict__ idx, const ClParams p,
                                                       uint64_t *__restrict__ hash, long long *__restrict__ status)
{
    const int64_t k = (int64_t)blockIdx.x * CL_LANES + (int)threadIdx.x;
    if (k >= p.n_records) return;
    ClRow r;
    const bool ok = cl_row(idx, k, p, &r);
    CL_ST_U64(hash, k, ok ? cl_hash(text, r) : 0ull);
    // (rare: the plain look first keeps a call that is wrong throughout from sending every record through one atomic)
    if (!ok && (long long)k < status[0]) __hip_atomic_fetch_min(status, (long long)k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// (the table and first[] carry no __restrict__: they are the two arrays other lanes change while this one runs, and only atomics
// touch them; everything that does carry it is read-only for the whole launch, or this lane's own slot[k])
__global__ __launch_bounds__(CL_LANES) void k_col_group(const uint8_t *__restrict__ text, const int64_t *__restrict__ idx,
                                                        const uint64_t *__restrict__ hash, const ClParams p,
                                                        const long long *__restrict__ status, int32_t *table, uint32_t *first,
                                                        int64_t *__restrict__ slot)
{
    const int64_t k = (int64_t)blockIdx.x * CL_LANES + (int)threadIdx.x;
    if (k >= p.n_records) return;
    if (status[0] != INT64_MAX) { CL_ST_SLOT(slot, k, CL_NO_SLOT); return; }      // a row failed its check: the call groups nothing
    ClProbe w;
    cl_probe_begin(idx, hash, k, p, &w);
    while (cl_probe_step(text, idx, hash, k, p, table, &w)) {}
    cl_probe_end(k, w, first, slot);
}

__global__ __launch_bounds__(CL_LANES) void k_col_rep(const uint32_t *__restrict__ first, const int64_t *__restrict__ slot, int64_t n,
                                                      int32_t *__restrict__ rep)
{
    const int64_t k = (int64_t)blockIdx.x * CL_LANES + (int)threadIdx.x;
    if (k < n) cl_rep(first, slot, k, rep);
}

}  // namespace

void mpb_launch_collapse(const uint8_t *text, const int64_t *idx, const ClParams &p, uint64_t *hash, int32_t *table, uint32_t *first,
                         int64_t *slot, int32_t *rep, int64_t *status, hipStream_t s)
{
    if (p.n_records <= 0) return;
    const dim3 grid((unsigned)((p.n_records + CL_LANES - 1) / CL_LANES)), block(CL_LANES);
    hipLaunchKernelGGL(k_col_hash, grid, block, 0, s, text, idx, p, hash, (long long *)status);
    hipLaunchKernelGGL(k_col_group, grid, block, 0, s, text, idx, hash, p, (const long long *)status, table, first, slot);
    hipLaunchKernelGGL(k_col_rep, grid, block, 0, s, first, slot, p.n_records, rep);
}
