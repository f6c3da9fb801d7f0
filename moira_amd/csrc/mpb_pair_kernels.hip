// mpb_pair_kernels.hip -- the step between two device-written FASTQ record indexes and k_contig's inputs (include/moira_pb.h,
// mpb_contigs_filter_fastq_host): pairing, the header comparison, validated pair descriptors, the LDS size classes and the class
// lists in pair order, a count / scan / scatter as the record index itself is one (mpb_index_kernels.hip):
//   k_pair_rows   one lane per candidate pair: row i of both indexes (not trusted) -> the mpb_pair_row mpb_pair_rows would write
//                 and its size class; the first pair whose rows fail a check and the first whose header tokens differ, each by
//                 an atomic min
//   k_pair_count  per workgroup of 256 pairs the count of every class (a ballot per class, the waves' counts through LDS) into
//                 table[workgroup][16]; the largest hdr_len + 2 (l1 + l2) of all pairs and the largest l1 + l2 of the pairs
//                 with a class by atomic max
//   k_pair_scan   one block: the exclusive prefix per class over the workgroups (trips of 64 workgroups with a carry), the
//                 class totals and the classes' first places in the list
//   k_pair_lists  the stable scatter: pair i -> list[first[class] + prefix[workgroup][class] + rank inside the workgroup]; every
//                 class list is ascending in pair number, as the host builds them
// What a lane does is mpb_pair_lane.inc (also compiled and checked on the host).  All results leave by plain vector stores and
// vector atomics; no workgroup waits for another; every loop runs over a header token, a table of fixed size, or the pairs.
// The four kernels have no timing id of their own: the host queues them inside MPB_K_CONTIG_ROWS' span.

#include "mpb_internal.h"

#define CD_FN __device__ __forceinline__
__device__ __forceinline__ int cd_gload8(const uint8_t *p) { return *p; }
#include "mpb_contig_args.h"

#define PR_FN __device__ __forceinline__
#define PR_LD_IDX(idx, k) ((idx)[k])
#define PR_LDB(text, i) ((uint32_t)(text)[i])
#include "mpb_pair_lane.inc"

static_assert(PR_LANES == 256 && PR_WAVE == 64 && PR_CLASS_SLOTS == MPB_LDS_CLASS_MAX && MPB_PAIR_HEAD_WORDS >= 2 * PR_CLASS_SLOTS,
              "the pairing step's shapes");

namespace {

__global__ __launch_bounds__(256) void k_pair_rows(const int64_t *__restrict__ fidx, const int64_t *__restrict__ ridx, int64_t m,
                                                   const uint8_t *__restrict__ ftext, int64_t fbytes, const uint8_t *__restrict__ rtext,
                                                   int64_t rbytes, int maxabs, int take, const MpbLdsClasses classes,
                                                   mpb_pair_row *__restrict__ rows, int8_t *__restrict__ cls, long long *__restrict__ status)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    mpb_pair_row r;
    bool ok = pr_row(fidx, ridx, i, fbytes, rbytes, &r);
    int64_t rho, rhl;
    ok = pr_hdr_range(ridx, i, rbytes, &rho, &rhl) && ok;
    if (!ok) { r.l1 = 0; r.l2 = 0; }
    rows[i] = r;
    cls[i] = (int8_t)(ok ? pr_class(r, fbytes, rbytes, maxabs, take, classes) : -1);
    // (rare, or settled after the first pair: the plain look first keeps a chunk from sending every pair through one atomic)
    if (!ok) {
        if ((long long)i < status[1]) __hip_atomic_fetch_min(status + 1, (long long)i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    if ((long long)i < status[0] && pr_hdr_differs(ftext, r.fhdr_off, r.hdr_len, rtext, rho, rhl))
        __hip_atomic_fetch_min(status + 0, (long long)i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ long long wave_max_i64(long long v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const long long o = __shfl_xor(v, d);
        v = o > v ? o : v;
    }
    return v;
}

// the ballots of the lane's wave per class into s_cnt[wave][class]; -> the ballot of the lane's own class (0 without one)
__device__ __forceinline__ unsigned long long pair_ballots(int c, uint32_t *s_cnt, int lane, int wv)
{
    unsigned long long mine = 0;
#pragma unroll
    for (int k = 0; k < PR_CLASS_SLOTS; k++) {
        const unsigned long long b = __ballot(c == k);
        if (lane == 0) s_cnt[wv * PR_CLASS_SLOTS + k] = (uint32_t)__popcll(b);
        if (c == k) mine = b;
    }
    return mine;
}

__global__ __launch_bounds__(PR_LANES) void k_pair_count(const mpb_pair_row *__restrict__ rows, const int8_t *__restrict__ cls, int64_t n,
                                                         uint32_t *__restrict__ table, long long *__restrict__ status)
{
    __shared__ uint32_t s_cnt[(PR_LANES / PR_WAVE) * PR_CLASS_SLOTS];
    const int tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t i = (int64_t)blockIdx.x * PR_LANES + tid;
    int c = -1;
    long long need = 0, both = 0;
    if (i < n) {
        const mpb_pair_row r = rows[i];
        c = cls[i];
        if (c >= PR_CLASS_SLOTS) c = -1;
        need = pr_need(r);
        if (c >= 0) both = (long long)r.l1 + r.l2;
    }
    (void)pair_ballots(c, s_cnt, lane, wv);
    need = wave_max_i64(need);
    both = wave_max_i64(both);
    if (lane == 0) {
        if (need > status[2]) __hip_atomic_fetch_max(status + 2, need, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (both > status[3]) __hip_atomic_fetch_max(status + 3, both, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    if (tid < PR_CLASS_SLOTS) {
        uint32_t sum = 0;
#pragma unroll
        for (int w = 0; w < PR_LANES / PR_WAVE; w++) sum += s_cnt[w * PR_CLASS_SLOTS + tid];
        table[(int64_t)blockIdx.x * PR_CLASS_SLOTS + tid] = sum;
    }
}

// prefix[g][k] = the pairs of class k in the workgroups before g; head[k] = the pairs of class k, head[16 + k] = the first place of
// class k in the list (the classes behind each other).  Thread t of a trip owns workgroup base + t / 16 and class t % 16.
__global__ __launch_bounds__(1024) void k_pair_scan(const uint32_t *__restrict__ table, int n_groups, uint32_t *__restrict__ prefix,
                                                    uint32_t *__restrict__ head)
{
    __shared__ uint32_t s_sum[1024];
    const int tid = (int)threadIdx.x, k = tid & (PR_CLASS_SLOTS - 1);
    uint32_t carry = 0;                                      // the class' pairs of the trips before (at most 2^31 pairs in a call)
    for (int base = 0; base < n_groups; base += 1024 / PR_CLASS_SLOTS) {
        const int g = base + tid / PR_CLASS_SLOTS;
        const uint32_t v = g < n_groups ? table[(int64_t)g * PR_CLASS_SLOTS + k] : 0u;
        s_sum[tid] = v;
        __syncthreads();
        for (int o = PR_CLASS_SLOTS; o < 1024; o <<= 1) {
            const uint32_t x = tid >= o ? s_sum[tid - o] : 0u;
            __syncthreads();
            s_sum[tid] += x;
            __syncthreads();
        }
        if (g < n_groups) prefix[(int64_t)g * PR_CLASS_SLOTS + k] = carry + s_sum[tid] - v;
        carry += s_sum[1024 - PR_CLASS_SLOTS + k];
        __syncthreads();                                     // (before the next trip overwrites s_sum)
    }
    s_sum[tid] = carry;
    __syncthreads();
    if (tid < PR_CLASS_SLOTS) {
        uint32_t first = 0;
        for (int j = 0; j < PR_CLASS_SLOTS; j++)
            if (j < tid) first += s_sum[j];
        head[tid] = carry;
        head[PR_CLASS_SLOTS + tid] = first;
    }
}

__global__ __launch_bounds__(PR_LANES) void k_pair_lists(const int8_t *__restrict__ cls, int64_t n, const uint32_t *__restrict__ prefix,
                                                         const uint32_t *__restrict__ head, int32_t *__restrict__ list)
{
    __shared__ uint32_t s_cnt[(PR_LANES / PR_WAVE) * PR_CLASS_SLOTS];
    const int tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t i = (int64_t)blockIdx.x * PR_LANES + tid;
    int c = i < n ? (int)cls[i] : -1;
    if (c >= PR_CLASS_SLOTS) c = -1;
    const unsigned long long mine = pair_ballots(c, s_cnt, lane, wv);
    __syncthreads();
    if (c < 0) return;
    const uint32_t rank = pr_rank(mine, lane, s_cnt, wv, c);
    const int64_t at = pr_list_slot(head[PR_CLASS_SLOTS + c], prefix[(int64_t)blockIdx.x * PR_CLASS_SLOTS + c], rank);
    if (at < n) list[at] = (int32_t)i;                       // (the list holds n entries: no more pairs have a class)
}

}  // namespace

void mpb_launch_pair_rows(const int64_t *fidx, const int64_t *ridx, int64_t m, const uint8_t *ftext, int64_t fbytes, const uint8_t *rtext,
                          int64_t rbytes, int maxabs, bool take, const MpbLdsClasses &classes, mpb_pair_row *rows, int8_t *cls,
                          int64_t *status, hipStream_t s)
{
    if (m <= 0) return;
    hipLaunchKernelGGL(k_pair_rows, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s, fidx, ridx, m, ftext, fbytes, rtext, rbytes, maxabs,
                       take ? 1 : 0, classes, rows, cls, (long long *)status);
}

void mpb_launch_pair_count(const mpb_pair_row *rows, const int8_t *cls, int64_t n, uint32_t *table, uint32_t *prefix, uint32_t *head,
                           int64_t *status, hipStream_t s)
{
    if (n <= 0) return;
    const int64_t groups = (n + PR_LANES - 1) / PR_LANES;
    hipLaunchKernelGGL(k_pair_count, dim3((unsigned)groups), dim3(PR_LANES), 0, s, rows, cls, n, table, (long long *)status);
    hipLaunchKernelGGL(k_pair_scan, dim3(1), dim3(1024), 0, s, table, (int)groups, prefix, head);
}

void mpb_launch_pair_lists(const int8_t *cls, int64_t n, const uint32_t *prefix, const uint32_t *head, int32_t *list, hipStream_t s)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_pair_lists, dim3((unsigned)((n + PR_LANES - 1) / PR_LANES)), dim3(PR_LANES), 0, s, cls, n, prefix, head, list);
}
