// mpb_index_kernels.hip -- the FASTQ record index on the device (include/moira_pb.h, mpb_fastq_index_host / mpb_filter_fastq_host).
// Record boundaries are a line-count property -- every four lines are a record, whatever they contain -- so the index is a
// count / scan / scatter / per-record pass, as mio_fastq_index_mt (csrc/fastio.cpp) builds it on the host's threads:
//   k_fq_lines   one workgroup per tile of FQ_TILE text bytes: the tile's newlines, and whether it holds a byte >= 0x80 or a
//                '\r' that no '\n' follows, before and behind the tile's last newline (mpb_index_lane.inc: the tile table)
//   k_fq_scan    one block: the exclusive prefix of the tiles' newlines (trips of 1024 tiles), then -- the total is known --
//                what the tiles' flags come to, and the head words {newlines, refusal flags, lines}
//   k_fq_starts  the text once more: start[L + 1] = p + 1 for the newline at byte p that ends line L, L = the tile's prefix + the
//                rank inside the tile (a workgroup scan of the lanes' counts) + the place inside the lane's word
//   k_fq_rows    one record per lane: the six columns of mio_fastq_index's row, the kind, k_pack_text's descriptor; the first
//                bad record by an atomic min, the longest packed length of a good one by an atomic max
// What a lane does is mpb_index_lane.inc (also compiled and checked on the host).  The text is read in whole aligned 16-byte
// words (its allocation holds round_up(text_bytes, 16) bytes) and no byte at or past text_bytes reaches a result.  No workgroup
// waits for another; every loop runs over the text, a line, or a table of fixed size.

#include "mpb_internal.h"

#define FQ_FN __device__ __forceinline__
typedef uint4 FqWord;
#define FQ_LDW(text, w) (*reinterpret_cast<const uint4 *>((text) + (int64_t)(w) * 16))
#define FQ_LDB(text, i) ((uint32_t)(text)[i])
#define FQ_LD_START(start, k) ((start)[k])
#define FQ_ST_START(start, k, v) ((start)[k] = (v))
#include "mpb_index_lane.inc"

static_assert(FQ_LANES == 256 && FQ_TILE == MPB_FQ_TILE && (uint32_t)FQ_TILE <= FQ_COUNT_MASK, "the indexer's shapes");

namespace {

// exclusive prefix of v over the 256 lanes of the workgroup, and the total (s_wsum: 4 words of LDS; two barriers)
__device__ __forceinline__ uint32_t fq_block_scan(uint32_t v, uint32_t *s_wsum, int tid, uint32_t *total)
{
    const int lane = tid & 63, wv = tid >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = (uint32_t)__shfl_up((int)inc, d);
        if (lane >= d) inc += o;
    }
    __syncthreads();                                         // (the previous trip's readers of s_wsum are done)
    if (lane == 63) s_wsum[wv] = inc;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) { const uint32_t s = s_wsum[k]; all += s; if (k < wv) before += s; }
    *total = all;
    return before + inc - v;
}

__global__ __launch_bounds__(FQ_LANES) void k_fq_lines(const uint8_t *__restrict__ text, int64_t text_bytes, int64_t n_tiles,
                                                       uint32_t *__restrict__ info)
{
    __shared__ uint32_t s_count, s_flags;
    __shared__ int s_last;
    const int64_t tile = blockIdx.x;
    if (tile >= n_tiles) return;
    const int tid = (int)threadIdx.x;
    if (tid == 0) { s_count = 0; s_flags = 0; s_last = 0; }
    __syncthreads();
    uint32_t na[FQ_TRIPS], cr[FQ_TRIPS];
    uint32_t count = 0;
    int last = 0;                                            // the lane's last newline, counted from the tile's start, plus one
#pragma unroll
    for (int t = 0; t < FQ_TRIPS; t++) {
        const int in_tile = (t * FQ_LANES + tid) * FQ_WORD_BYTES;
        const int64_t w = tile * FQ_TILE_WORDS + t * FQ_LANES + tid;
        uint32_t nl = 0;
        na[t] = 0; cr[t] = 0;
        if (w * FQ_WORD_BYTES < text_bytes) fq_scan_word(text, text_bytes, w, &nl, &na[t], &cr[t]);
        count += (uint32_t)__popc(nl);
        if (nl) last = in_tile + (32 - __clz((int)nl));
    }
    // the workgroup's sum and its last newline: one lane per wave after the wave's own reduction
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        count += (uint32_t)__shfl_xor((int)count, d);
        last = max(last, __shfl_xor(last, d));
    }
    if ((tid & 63) == 0) { atomicAdd(&s_count, count); atomicMax(&s_last, last); }
    __syncthreads();
    const int last_nl1 = s_last;
    uint32_t f = 0;
#pragma unroll
    for (int t = 0; t < FQ_TRIPS; t++) f |= fq_word_flags(na[t], cr[t], (t * FQ_LANES + tid) * FQ_WORD_BYTES, last_nl1);
    if (f) atomicOr(&s_flags, f);                            // (rare)
    __syncthreads();
    if (tid == 0) info[tile] = s_count | s_flags;
}

// prefix[t] = the newlines before tile t; head[0] = the newlines of the text, head[1] = the refusal flags (bit 0: a non-ASCII
// byte, bit 1: a lone carriage return, among the bytes the host would look at), head[2] = the lines: one more than the newlines
// when the text is final and its last byte is no newline
__global__ __launch_bounds__(1024) void k_fq_scan(const uint8_t *__restrict__ text, int64_t text_bytes, int final_text,
                                                  const uint32_t *__restrict__ info, int n_tiles, uint32_t *__restrict__ prefix,
                                                  uint32_t *__restrict__ head)
{
    __shared__ uint32_t s_sum[1024];
    __shared__ uint32_t s_flags;
    const int tid = (int)threadIdx.x;
    if (tid == 0) s_flags = 0;
    uint32_t carry = 0;                                      // the newlines of the trips before (at most 2^30: a text is 1 GiB)
    for (int base = 0; base < n_tiles; base += 1024) {
        const int t = base + tid;
        const uint32_t v = t < n_tiles ? info[t] & FQ_COUNT_MASK : 0u;
        s_sum[tid] = v;
        __syncthreads();
        for (int o = 1; o < 1024; o <<= 1) {
            const uint32_t x = tid >= o ? s_sum[tid - o] : 0u;
            __syncthreads();
            s_sum[tid] += x;
            __syncthreads();
        }
        if (t < n_tiles) prefix[t] = carry + s_sum[tid] - v;
        carry += s_sum[1023];
        __syncthreads();                                     // (before the next trip overwrites s_sum)
    }
    const uint32_t total = carry;
    uint32_t f = 0;
    for (int t = tid; t < n_tiles; t += 1024) {
        const uint32_t w = info[t];
        const uint32_t before = prefix[t];                   // (this thread's own store of the loop above: t = tid mod 1024)
        f |= fq_tile_refusal(w, final_text != 0 || total - before - (w & FQ_COUNT_MASK) > 0u);
    }
    if (f) atomicOr(&s_flags, f);
    __syncthreads();
    if (tid == 0) {
        uint32_t lines = total;
        if (final_text && text_bytes > 0) {
            const int64_t p = text_bytes - 1;
            const FqWord v = FQ_LDW(text, p >> 4);
            const uint32_t x[4] = {v.x, v.y, v.z, v.w};
            if (((x[(p & 15) >> 2] >> (8 * (p & 3))) & 0xffu) != 0x0au) lines++;
        }
        head[0] = total; head[1] = s_flags; head[2] = lines;
    }
}

__global__ __launch_bounds__(FQ_LANES) void k_fq_starts(const uint8_t *__restrict__ text, int64_t text_bytes, int64_t n_tiles,
                                                        const uint32_t *__restrict__ prefix, const uint32_t *__restrict__ head,
                                                        uint32_t *__restrict__ start, int64_t n_start)
{
    __shared__ uint32_t s_wsum[4];
    const int64_t tile = blockIdx.x;
    if (tile >= n_tiles) return;
    const int tid = (int)threadIdx.x;
    int64_t line = prefix[tile];                             // the line that the tile's first newline ends
    if (tile == 0 && tid == 0) {
        if (n_start > 0) start[0] = 0;
        const int64_t newlines = head[0], lines = head[2];   // an unterminated last line of a final text ends at the text's end
        if (lines > newlines && lines < n_start) start[lines] = (uint32_t)text_bytes;
    }
    if (line + 1 >= n_start) return;                         // (uniform: nothing of this tile is stored)
#pragma unroll
    for (int t = 0; t < FQ_TRIPS; t++) {
        const int64_t w = tile * FQ_TILE_WORDS + t * FQ_LANES + tid;
        uint32_t nl = 0, na, cr;
        if (w * FQ_WORD_BYTES < text_bytes) fq_scan_word(text, text_bytes, w, &nl, &na, &cr);
        uint32_t trip;
        const uint32_t rank = fq_block_scan((uint32_t)__popc(nl), s_wsum, tid, &trip);
        if (nl) fq_store_starts(start, n_start, w, nl, line + rank);
        line += trip;
    }
}

// status[0] = the first record that fails one of the three checks (atomic min; INT64_MAX: none), status[1] = the longest packed
// length of a record that passes them (atomic max), status[2] = 1 when a record's line starts failed their check
__global__ __launch_bounds__(256) void k_fq_rows(const uint8_t *__restrict__ text, int64_t text_bytes, const uint32_t *__restrict__ start,
                                                 int64_t n_start, int64_t n, int32_t max_len, int64_t *__restrict__ idx,
                                                 uint8_t *__restrict__ kinds, mpb_text_row *__restrict__ desc, long long *__restrict__ status)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    int64_t row[6];
    int32_t kind = FQ_REC_OK;
    mpb_text_row d;
    d.seq_off = 0; d.qual_off = 0; d.len = -1; d.pad = 0;
    const bool ok = fq_row(text, text_bytes, start, n_start, r, max_len, row, &kind, &d);
    if (!ok) {
#pragma unroll
        for (int k = 0; k < 6; k++) row[k] = 0;
        __hip_atomic_fetch_max(status + 2, 1ll, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
#pragma unroll
    for (int k = 0; k < 6; k++) idx[r * 6 + k] = row[k];
    kinds[r] = (uint8_t)kind;
    desc[r] = d;
    if (!ok) return;
    // (rare, or settled after a few records: the plain look first keeps a chunk from sending every record through one atomic)
    if (kind != FQ_REC_OK) {
        if ((long long)r < status[0]) __hip_atomic_fetch_min(status + 0, (long long)r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else if ((long long)d.len > status[1]) {
        __hip_atomic_fetch_max(status + 1, (long long)d.len, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

}  // namespace

void mpb_launch_fq_lines(const uint8_t *text, int64_t text_bytes, int64_t n_tiles, uint32_t *info, hipStream_t s)
{
    if (n_tiles <= 0) return;
    hipLaunchKernelGGL(k_fq_lines, dim3((unsigned)n_tiles), dim3(FQ_LANES), 0, s, text, text_bytes, n_tiles, info);
}

void mpb_launch_fq_scan(const uint8_t *text, int64_t text_bytes, bool final_text, const uint32_t *info, int64_t n_tiles,
                        uint32_t *prefix, uint32_t *head, hipStream_t s)
{
    hipLaunchKernelGGL(k_fq_scan, dim3(1), dim3(1024), 0, s, text, text_bytes, final_text ? 1 : 0, info, (int)n_tiles, prefix, head);
}

void mpb_launch_fq_starts(const uint8_t *text, int64_t text_bytes, int64_t n_tiles, const uint32_t *prefix, const uint32_t *head,
                          uint32_t *start, int64_t n_start, hipStream_t s)
{
    if (n_tiles <= 0) return;
    hipLaunchKernelGGL(k_fq_starts, dim3((unsigned)n_tiles), dim3(FQ_LANES), 0, s, text, text_bytes, n_tiles, prefix, head, start, n_start);
}

void mpb_launch_fq_rows(const uint8_t *text, int64_t text_bytes, const uint32_t *start, int64_t n_start, int64_t n, int32_t max_len,
                        int64_t *idx, uint8_t *kinds, mpb_text_row *desc, int64_t *status, hipStream_t s)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_fq_rows, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, text, text_bytes, start, n_start, n, max_len, idx,
                       kinds, desc, (long long *)status);
}
