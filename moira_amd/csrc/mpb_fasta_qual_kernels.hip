// mpb_fasta_qual_kernels.hip -- fasta+qual input on the device (include/moira_pb.h, mpb_fasta_qual_index_host /
// mpb_filter_fasta_qual_host): two texts become the `header token | sequence | quality bytes` buffer and the six-column index that
// mio_fasta_qual_index builds on the host (csrc/fastio.cpp).  Both texts first go through the line kernels of the FASTQ index
// (mpb_index_kernels.hip: they count newlines, flag what the byte-level path declines and write line starts, whatever the lines
// hold); record r is lines 2 r and 2 r + 1 of each.  Then a count / prefix / write, as the formatter (mpb_format_kernels.hip) is:
//   k_fa_count   FA_GROUP lanes per record: the line starts by fq_row's check (they are device-written and not trusted), the four
//                lines stripped, the header tokens compared, the quality line's grammar by byte-class masks, 16 aligned bytes
//                per lane and step, its separators counted; size[r] = the record's slot, header token + 2 x sequence; the first
//                record that is not taken, with its reason, by an atomic min into status[0]
//   k_fa_scan    one block: prefix[0 .. n] = the exclusive prefix of size (trips of 1024 with a carry); head = {n_fit, out_used}:
//                the leading records whose slots end at or before out_cap, and where the last of them ends
//   k_fa_write   the same lanes per record, r < n_fit: header token and sequence copied into the slot, every quality token parsed
//                into one byte at its rank -- the separators before it: an exclusive scan of the group's counts plus a running
//                base; the index row, k_pack_text's descriptor, the longest packed length by an atomic max.  Nothing is written
//                when status[0] is set: one bad record hands the whole call back.
// What a lane does is mpb_fasta_qual_lane.inc (also compiled and checked on the host).  The texts are read in whole aligned
// 16-byte words (their allocations hold round_up(bytes, 16)) and no byte at or past text_bytes reaches a result; stores into out
// stay inside the record's own slot.  All results leave by plain vector stores and vector atomics; no workgroup waits for
// another; every loop runs over a line or a table of fixed size.
// The three kernels have no timing id of their own: the host queues them inside MPB_K_FQ_ROWS' span.

#include "mpb_internal.h"

struct FaOutDev { uint8_t *p; int64_t lo, hi; };             // the record's own slot [lo, hi) of out

#define FQ_FN __device__ __forceinline__
typedef uint4 FqWord;
#define FQ_LDW(text, w) (*reinterpret_cast<const uint4 *>((text) + (int64_t)(w) * 16))
#define FQ_LDB(text, i) ((uint32_t)(text)[i])
#define FQ_LD_START(start, k) ((start)[k])
#define FQ_ST_START(start, k, v) ((start)[k] = (v))
#define FA_FN __device__ __forceinline__
#define FA_ST8(o, pos, b)                                                                   \
    do {                                                                                    \
        const int64_t pos_ = (pos);                                                         \
        if (pos_ >= (o).lo && pos_ < (o).hi) (o).p[pos_] = (uint8_t)(b);                    \
    } while (0)
#include "mpb_fasta_qual_lane.inc"

static_assert(FA_LANES == 256 && FA_GROUP == 8 && FA_STRIDE == 128, "the fasta+qual stage's shapes");

namespace {

// status[0] = the key (fa_key) of the first record that is not taken (atomic min; INT64_MAX: none)
__global__ __launch_bounds__(FA_LANES) void k_fa_count(const uint8_t *__restrict__ ftext, int64_t fbytes,
                                                       const uint32_t *__restrict__ fstart, const uint8_t *__restrict__ qtext,
                                                       int64_t qbytes, const uint32_t *__restrict__ qstart, int64_t n_start,
                                                       int64_t n, int64_t *__restrict__ size, long long *__restrict__ status)
{
    const int sub = (int)threadIdx.x & (FA_GROUP - 1);
    const int64_t r = (int64_t)blockIdx.x * (FA_LANES / FA_GROUP) + ((int)threadIdx.x / FA_GROUP);
    if (r >= n) return;                                      // (a whole group leaves or stays)
    FaRec rec;
    int which;
    int why = fa_record(ftext, fbytes, fstart, n_start, qtext, qbytes, qstart, n_start, r, true, &rec, &which);
    if (why == 0) {                                          // (the group's lanes agree: the record is theirs in common)
        bool bad;
        long long seps = fa_count_lane(qtext, rec, sub, &bad);
        int any = bad ? 1 : 0;
#pragma unroll
        for (int d = 1; d < FA_GROUP; d <<= 1) {
            seps += __shfl_xor(seps, d);
            any |= __shfl_xor(any, d);
        }
        why = fa_verdict(rec, any != 0, seps);
        which = 1;
    }
    if (sub != 0) return;
    size[r] = why == 0 ? fa_slot_bytes(rec) : 0;
    if (why != 0) {
        // (rare: the plain look first keeps texts that are wrong throughout from sending every record through one atomic)
        const long long key = fa_key(r, why, which);
        if (key < status[0]) __hip_atomic_fetch_min(status, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// prefix[r] = the bytes of the slots before r, prefix[n] = all of them; head[0] = n_fit, head[1] = prefix[n_fit]
__global__ __launch_bounds__(1024) void k_fa_scan(const int64_t *__restrict__ size, int64_t n, int64_t out_cap,
                                                  int64_t *__restrict__ prefix, int64_t *__restrict__ head)
{
    __shared__ int64_t s_sum[1024];
    __shared__ unsigned long long s_fit;
    const int tid = (int)threadIdx.x;
    if (tid == 0) s_fit = 0;
    int64_t carry = 0;
    unsigned long long fit = 0;                              // records of this lane whose slots end inside out_cap
    for (int64_t base = 0; base < n; base += 1024) {
        const int64_t k = base + tid;
        const int64_t v = k < n ? size[k] : 0;
        s_sum[tid] = v;
        __syncthreads();
        for (int o = 1; o < 1024; o <<= 1) {
            const int64_t x = tid >= o ? s_sum[tid - o] : 0;
            __syncthreads();
            s_sum[tid] += x;
            __syncthreads();
        }
        if (k < n) {
            prefix[k] = carry + s_sum[tid] - v;
            if (carry + s_sum[tid] <= out_cap) fit++;        // (sizes are >= 0, so the ends ascend: these are leading records)
        }
        carry += s_sum[1023];
        __syncthreads();                                     // (before the next trip overwrites s_sum)
    }
    if (fit) atomicAdd(&s_fit, fit);
    if (tid == 0) prefix[n] = carry;
    __syncthreads();                                         // (s_fit is whole; this block's prefix stores are visible to it)
    if (tid == 0) {
        const int64_t n_fit = (int64_t)s_fit;
        head[0] = n_fit; head[1] = prefix[n_fit]; head[2] = carry; head[3] = 0;
    }
}

// status[1] = the longest packed length of a written record (atomic max), status[2] = 1 when a slot's place failed its check
__global__ __launch_bounds__(FA_LANES) void k_fa_write(const uint8_t *__restrict__ ftext, int64_t fbytes,
                                                       const uint32_t *__restrict__ fstart, const uint8_t *__restrict__ qtext,
                                                       int64_t qbytes, const uint32_t *__restrict__ qstart, int64_t n_start,
                                                       int64_t n, int32_t max_len, const int64_t *__restrict__ prefix,
                                                       const int64_t *__restrict__ head, uint8_t *__restrict__ out,
                                                       int64_t out_bytes, int64_t *__restrict__ idx,
                                                       mpb_text_row *__restrict__ desc, long long *__restrict__ status)
{
    if (status[0] != INT64_MAX) return;                      // a record is not taken: the call writes nothing
    const int sub = (int)threadIdx.x & (FA_GROUP - 1);
    const int64_t r = (int64_t)blockIdx.x * (FA_LANES / FA_GROUP) + ((int)threadIdx.x / FA_GROUP);
    int64_t n_fit = head[0];
    if (n_fit > n) n_fit = n;
    if (r >= n_fit) return;
    FaRec rec;
    int which;
    if (fa_record(ftext, fbytes, fstart, n_start, qtext, qbytes, qstart, n_start, r, false, &rec, &which) != 0) return;   // (k_fa_count said so already)
    const int64_t at = prefix[r], bytes = fa_slot_bytes(rec);
    if (at < 0 || bytes > out_bytes || at > out_bytes - bytes) {                         // prefix[] is device-written as well
        if (sub == 0) __hip_atomic_fetch_max(status + 2, 1ll, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    FaOutDev o{out, at, at + bytes};
    fa_copy(ftext, rec.hdr_off, rec.hdr_len, sub, o, at);
    fa_copy(ftext, rec.seq_off, rec.seq_len, sub, o, at + rec.hdr_len);
    const int64_t qat = at + rec.hdr_len + rec.seq_len;
    const int64_t w1 = fa_end_word(rec);
    int64_t before = 0;                                      // the separators of the steps before
    for (int64_t w0 = fa_first_word(rec); w0 < w1; w0 += FA_GROUP) {
        const int64_t w = w0 + sub;
        FaQ q;
        int mine = 0;
        if (w < w1) { fa_qload(qtext, rec, w, &q); mine = fa_qseps(q); }
        int incl = mine;                                     // the inclusive scan over the group's lanes
#pragma unroll
        for (int d = 1; d < FA_GROUP; d <<= 1) {
            const int x = __shfl_up(incl, d, FA_GROUP);
            if (sub >= d) incl += x;
        }
        const int total = __shfl(incl, FA_GROUP - 1, FA_GROUP);
        if (w < w1) fa_qstore(q, rec, before + (incl - mine), o, qat);
        before += total;
    }
    if (sub != 0) return;
    int64_t row[6];
    mpb_text_row d;
    fa_row_out(rec, at, max_len, row, &d);
#pragma unroll
    for (int k = 0; k < 6; k++) idx[r * 6 + k] = row[k];
    desc[r] = d;
    if ((long long)d.len > status[1]) __hip_atomic_fetch_max(status + 1, (long long)d.len, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace

void mpb_launch_fa_count(const uint8_t *ftext, int64_t fbytes, const uint32_t *fstart, const uint8_t *qtext, int64_t qbytes,
                         const uint32_t *qstart, int64_t n_start, int64_t n, int64_t out_cap, int64_t *size, int64_t *prefix,
                         int64_t *head, int64_t *status, hipStream_t s)
{
    if (n > 0) {
        const int64_t per = FA_LANES / FA_GROUP;
        hipLaunchKernelGGL(k_fa_count, dim3((unsigned)((n + per - 1) / per)), dim3(FA_LANES), 0, s, ftext, fbytes, fstart, qtext, qbytes,
                           qstart, n_start, n, size, (long long *)status);
    }
    hipLaunchKernelGGL(k_fa_scan, dim3(1), dim3(1024), 0, s, size, n, out_cap, prefix, head);
}

void mpb_launch_fa_write(const uint8_t *ftext, int64_t fbytes, const uint32_t *fstart, const uint8_t *qtext, int64_t qbytes,
                         const uint32_t *qstart, int64_t n_start, int64_t n, int32_t max_len, const int64_t *prefix, const int64_t *head,
                         uint8_t *out, int64_t out_bytes, int64_t *idx, mpb_text_row *desc, int64_t *status, hipStream_t s)
{
    if (n <= 0) return;
    const int64_t per = FA_LANES / FA_GROUP;
    hipLaunchKernelGGL(k_fa_write, dim3((unsigned)((n + per - 1) / per)), dim3(FA_LANES), 0, s, ftext, fbytes, fstart, qtext, qbytes,
                       qstart, n_start, n, max_len, prefix, head, out, out_bytes, idx, desc, (long long *)status);
}
