// mpb_format_kernels.hip -- the writer's formatter on the device (include/moira_pb.h, mpb_format_records_host): records sel[k] of a
// text and its record index become fasta, qual or fastq text or contigs.report lines, with or without the ";ee=..;size=1;"
// suffix, byte for byte what mio_format and mio_format_report write (csrc/fastio.cpp).  A count /
// prefix / write, as the record index (mpb_index_kernels.hip) and the pairing step (mpb_pair_kernels.hip) are:
//   k_fmt_count  FM_GROUP lanes per selected record: the row by every check (it is not trusted, uploaded or device-written), the
//                output bytes of the record into size[k] -- arithmetic on the row for FASTA and FASTQ, plus digit counts for the
//                suffix and a report line's three numbers (aux, by record; ee, by position: integer work on its bits, and a
//                value outside the taken domain fails the row); for QUAL the values >= 10
//                and >= 100 after the clamp, counted 16 bytes per lane and step; the first k whose row fails a check by an
//                atomic min into status[0]
//   k_fmt_scan   one block: prefix[0 .. n] = the exclusive prefix of size (trips of 1024 with a carry), head[0] = the total
//   k_fmt_write  FM_GROUP lanes per record of a range of k: the record at prefix[k], clipped to the window of the formatted text
//                the call asked for; header, label, sequence and quality string move in 16-byte words per lane (aligned fetch
//                and funnel on the source side, as k_pack_text has them); QUAL values are rendered 16 per lane and step and
//                placed by an exclusive scan of the group's byte counts plus a running base; relabel_index, the suffix and a
//                report line's numbers are rendered by one lane each.  Nothing is written when status[0]
//                is set.  The output is stored by bytes (DESIGN 4o says why).
// What a lane does is mpb_format_lane.inc (also compiled and checked on the host).  All results leave by plain vector stores and
// vector atomics; no workgroup waits for another; every loop runs over a checked length or a fixed table.
// The three kernels have no timing id of their own: the host queues them inside MPB_K_PACK_TEXT's span.

#include "mpb_internal.h"

struct FmOutDev { uint8_t *p; int64_t base, lo, hi; };       // p[pos - base] for lo <= pos < hi: the window and the record's own range

#define FM_FN __device__ __forceinline__
#define FM_LD_I64(p, k) ((p)[k])
#define FM_LD_I32(p, k) ((p)[k])
#define FM_LD_U64(p, k) ((p)[k])
#define FM_LD16(text, off) fm_gload16((text) + (off))
#define FM_ST8(o, pos, b)                                                                   \
    do {                                                                                    \
        const int64_t pos_ = (pos);                                                         \
        if (pos_ >= (o).lo && pos_ < (o).hi) (o).p[pos_ - (o).base] = (uint8_t)(b);         \
    } while (0)
struct fm_w16;
__device__ __forceinline__ fm_w16 fm_gload16(const uint8_t *p);
#include "mpb_format_lane.inc"
__device__ __forceinline__ fm_w16 fm_gload16(const uint8_t *p)
{
    const uint4 v = *reinterpret_cast<const uint4 *>(p);
    fm_w16 o;
    o.w[0] = v.x; o.w[1] = v.y; o.w[2] = v.z; o.w[3] = v.w;
    return o;
}

static_assert(FM_LANES == 256 && FM_GROUP == 8 && sizeof(FmParams) <= 128, "the formatter's shapes");

namespace {

// the sum over the FM_GROUP lanes of a record (all of them are here: k is theirs in common)
__device__ __forceinline__ uint64_t group_sum_u64(uint64_t v)
{
#pragma unroll
    for (int d = 1; d < FM_GROUP; d <<= 1) v += (uint64_t)__shfl_xor((long long)v, d);
    return v;
}

__global__ __launch_bounds__(FM_LANES) void k_fmt_count(const uint8_t *__restrict__ text, const int64_t *__restrict__ idx,
                                                        const int64_t *__restrict__ sel, const int64_t *__restrict__ relabel_index,
                                                        const int32_t *__restrict__ label_id, const uint64_t *__restrict__ ee,
                                                        const int32_t *__restrict__ aux0, const int32_t *__restrict__ aux1,
                                                        const int32_t *__restrict__ aux2, int64_t nsel, const FmParams p,
                                                        int64_t *__restrict__ size, long long *__restrict__ status)
{
    const int sub = (int)threadIdx.x & (FM_GROUP - 1);
    const int64_t k = (int64_t)blockIdx.x * (FM_LANES / FM_GROUP) + ((int)threadIdx.x / FM_GROUP);
    if (k >= nsel) return;                                   // (a whole group leaves or stays)
    FmRow r;
    FmExtra x;
    const bool ok = fm_rec_row(idx, sel, relabel_index, label_id, ee, aux0, aux1, aux2, k, p, &r, &x);
    uint64_t counts = 0;
    if (ok && p.kind == FM_KIND_QUAL) counts = group_sum_u64(fm_count_lane(text, r, sub, p));
    if (sub != 0) return;
    size[k] = ok ? fm_size_x(r, x, counts, p) : 0;
    // (rare: the plain look first keeps a call that is wrong throughout from sending every record through one atomic)
    if (!ok && (long long)k < status[0]) __hip_atomic_fetch_min(status, (long long)k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// prefix[k] = the bytes of the records before k, prefix[n] = head[0] = all of them
__global__ __launch_bounds__(1024) void k_fmt_scan(const int64_t *__restrict__ size, int64_t n, int64_t *__restrict__ prefix,
                                                   int64_t *__restrict__ head)
{
    __shared__ int64_t s_sum[1024];
    const int tid = (int)threadIdx.x;
    int64_t carry = 0;
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
        if (k < n) prefix[k] = carry + s_sum[tid] - v;
        carry += s_sum[1023];
        __syncthreads();                                     // (before the next trip overwrites s_sum)
    }
    if (tid == 0) { prefix[n] = carry; head[0] = carry; }
}

__global__ __launch_bounds__(FM_LANES) void k_fmt_write(const uint8_t *__restrict__ text, const uint8_t *__restrict__ blob,
                                                        const int64_t *__restrict__ idx, const int64_t *__restrict__ sel,
                                                        const int64_t *__restrict__ relabel_index, const int32_t *__restrict__ label_id,
                                                        const uint64_t *__restrict__ ee, const int32_t *__restrict__ aux0,
                                                        const int32_t *__restrict__ aux1, const int32_t *__restrict__ aux2,
                                                        int64_t k0, int64_t k1, const FmParams p, const int64_t *__restrict__ prefix,
                                                        const long long *__restrict__ status, int64_t win_lo, int64_t win_hi,
                                                        uint8_t *__restrict__ out)
{
    if (status[0] != INT64_MAX) return;                      // a row failed its check: the call writes nothing
    const int sub = (int)threadIdx.x & (FM_GROUP - 1);
    const int64_t k = k0 + (int64_t)blockIdx.x * (FM_LANES / FM_GROUP) + ((int)threadIdx.x / FM_GROUP);
    if (k >= k1) return;
    FmRow r;
    FmExtra x;
    if (!fm_rec_row(idx, sel, relabel_index, label_id, ee, aux0, aux1, aux2, k, p, &r, &x)) return;      // (k_fmt_count said so already)
    const int64_t at = prefix[k], end = prefix[k + 1];
    FmOutDev o{out, win_lo, at > win_lo ? at : win_lo, end < win_hi ? end : win_hi};
    if (o.lo >= o.hi) return;
    int64_t w = at + fm_write_header_x(text, blob, r, x, sub, p, o, at);
    if (p.kind == FM_KIND_REPORT) return;
    if (p.kind != FM_KIND_QUAL) { fm_write_lines(text, r, sub, p, o, w); return; }
    const int steps = (r.L + 16 * FM_GROUP - 1) / (16 * FM_GROUP);
    for (int s = 0; s < steps; s++) {
        int nv;
        const fm_w16 ql = fm_qual_word(text, r, s, sub, &nv);
        const bool first = s == 0 && sub == 0;
        const int mine = fm_qual_bytes16(ql, nv, first, p);
        int incl = mine;                                     // the inclusive scan over the group's lanes
#pragma unroll
        for (int d = 1; d < FM_GROUP; d <<= 1) {
            const int x = __shfl_up(incl, d, FM_GROUP);
            if (sub >= d) incl += x;
        }
        const int total = __shfl(incl, FM_GROUP - 1, FM_GROUP);
        fm_qual_render16(ql, nv, first, p, o, w + (incl - mine));
        w += total;
    }
    if (sub == 0) FM_ST8(o, w, (uint32_t)'\n');
}

}  // namespace

void mpb_launch_fmt_count(const uint8_t *text, const int64_t *idx, const int64_t *sel, const int64_t *relabel_index,
                          const int32_t *label_id, const uint64_t *ee, const int32_t *const aux[3], int64_t nsel, const FmParams &p, int64_t *size, int64_t *prefix, int64_t *head,
                          int64_t *status, hipStream_t s)
{
    if (nsel > 0) {
        const int64_t per = FM_LANES / FM_GROUP;
        hipLaunchKernelGGL(k_fmt_count, dim3((unsigned)((nsel + per - 1) / per)), dim3(FM_LANES), 0, s, text, idx, sel, relabel_index,
                           label_id, ee, aux[0], aux[1], aux[2], nsel, p, size, (long long *)status);
    }
    hipLaunchKernelGGL(k_fmt_scan, dim3(1), dim3(1024), 0, s, size, nsel, prefix, head);
}

void mpb_launch_fmt_write(const uint8_t *text, const uint8_t *blob, const int64_t *idx, const int64_t *sel,
                          const int64_t *relabel_index, const int32_t *label_id, const uint64_t *ee, const int32_t *const aux[3],
                          int64_t k0, int64_t k1, const FmParams &p,
                          const int64_t *prefix, const int64_t *status, int64_t win_lo, int64_t win_hi, uint8_t *out, hipStream_t s)
{
    if (k1 <= k0 || win_hi <= win_lo) return;
    const int64_t per = FM_LANES / FM_GROUP;
    hipLaunchKernelGGL(k_fmt_write, dim3((unsigned)((k1 - k0 + per - 1) / per)), dim3(FM_LANES), 0, s, text, blob, idx, sel,
                       relabel_index, label_id, ee, aux[0], aux[1], aux[2], k0, k1, p, prefix, (const long long *)status, win_lo, win_hi, out);
}
