// mpb_inflate_kernels.hip -- BGZF .gz input on the device (include/moira_pb.h, mpb_bgzf_inflate_host): k_bgzf_inflate inflates one
// BGZF member per workgroup of 64 lanes (one wave) from its validated row {stream_off, out_off, stream_len, out_len}.  What a lane
// does, and the order in which the wave does it, is mpb_inflate_lane.inc (bi_member; also compiled and checked on the host); here
// are the device forms of its loads, stores and fences, the recheck of the row against the piece's buffers, and the status words.
//
//   window  the member's whole text, 64 KiB of LDS (ISIZE may be 65,536); literals are byte stores of lane 0, a match is copied by
//           the lanes together, 64 bytes per step, from bytes that all lie before the match
//   ring    the compressed bytes are never read from global memory per refill: two halves of 1 KiB in LDS, each filled by the wave
//           with one range-checked 16-byte load per lane before the bit reader gets there; bytes past the stream read as zero, and
//           the consumed bits are checked against 8 * stream_len
//   tables  a fast table per code (10 / 8 / 7 index bits for literal-length / distance / code-length codes) and the canonical
//           count / sorted arrays behind it for longer codes, built by the lanes together per dynamic block; the fixed code's own
//           pair is built once per member, when a fixed block appears
//   end     a member is taken only when its final block ended at exactly out_len bytes with the stream used up to its last byte;
//           only then is the window stored to text + out_off, 16 bytes per lane
// One wave per workgroup: no __syncthreads; the lanes' LDS traffic is ordered by a workgroup-scope fence (BI_SYNC).  No workgroup
// waits for another; the symbol loop consumes at least a bit per turn and is capped at 8 * stream_len + 8 turns besides.
// LDS: 65,536 (window) + 9,724 (ring, tables, code lengths) = 75,260 bytes of the 81,920 that let two workgroups share a CU.

#include "mpb_internal.h"

#define BI_FN __device__ __forceinline__
__device__ __forceinline__ void bi_ld_in16(const uint8_t *in, int64_t q, uint32_t *w)
{
    const uint4 v = *(const uint4 *)(in + q);                // (q is a multiple of 16 and `in` a 256-byte aligned block)
    w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
}
__device__ __forceinline__ void bi_st_out16(uint8_t *text, int64_t q, const uint32_t *w)
{
    *(uint4 *)(text + q) = make_uint4(w[0], w[1], w[2], w[3]);
}
#define BI_LD_IN16(in, q, w) bi_ld_in16((in), (q), (w))
#define BI_LD_IN8(in, q) ((in)[q])
#define BI_ST_OUT16(text, q, w) bi_st_out16((text), (q), (w))
#define BI_ST_OUT8(text, q, b) ((text)[q] = (b))
#define BI_ATOMIC_INC(ptr) atomicAdd((ptr), 1u)
#define BI_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup"); __builtin_amdgcn_wave_barrier(); } while (0)
#define BI_STATES 1
#define BI_EACH(lane, lane0) for (int lane = (lane0), bi_once_ = 1; bi_once_; bi_once_ = 0)
#define BI_I(lane) 0
#include "mpb_inflate_lane.inc"

static_assert(BI_OK == MPB_BGZF_WHY_OK && BI_HEADER == MPB_BGZF_WHY_HEADER && BI_BTYPE == MPB_BGZF_WHY_BLOCK_TYPE &&
              BI_STORED == MPB_BGZF_WHY_STORED_LENGTH && BI_CLCODE == MPB_BGZF_WHY_CODE_LENGTH_CODE && BI_REPEAT == MPB_BGZF_WHY_REPEAT &&
              BI_TREE == MPB_BGZF_WHY_TREE && BI_SYMBOL == MPB_BGZF_WHY_SYMBOL && BI_DISTANCE == MPB_BGZF_WHY_DISTANCE &&
              BI_OVERRUN == MPB_BGZF_WHY_OVERRUN && BI_SHORT == MPB_BGZF_WHY_SHORT && BI_TRUNCATED == MPB_BGZF_WHY_TRUNCATED &&
              BI_TRAILING == MPB_BGZF_WHY_TRAILING_BYTES && BI_CRC == MPB_BGZF_WHY_CRC, "the why codes of the lane code and the header");
static_assert(sizeof(BiShared) + BI_WINDOW <= 81920, "two workgroups of k_bgzf_inflate per CU");
static_assert(MPB_INFLATE_MSTAT == 8, "k_bgzf_inflate's status row");

namespace {

__global__ __launch_bounds__(BI_LANES) void k_bgzf_inflate(const uint8_t *__restrict__ in, int64_t in_bytes,
                                                            const mpb_bgzf_member_row *__restrict__ rows, int64_t n_members,
                                                            uint8_t *__restrict__ text, int64_t text_bytes, uint32_t *__restrict__ mstat)
{
    __shared__ __align__(16) uint32_t s_window[BI_WINDOW / 4];
    __shared__ __align__(16) BiShared s_sh;

    const int64_t m = blockIdx.x;
    if (m >= n_members) return;
    const int lane = (int)threadIdx.x;
    const mpb_bgzf_member_row r = rows[m];
    uint32_t *st = mstat + m * MPB_INFLATE_MSTAT;
    // the row again, against this piece's buffers: every index below derives from these four checked values
    const bool ok = r.out_len >= 0 && r.out_len <= BI_WINDOW && r.out_off >= 0 && r.out_off <= text_bytes - (int64_t)r.out_len &&
                    r.stream_len >= 0 && r.stream_len <= 65536 && r.stream_off >= 0 && r.stream_off <= in_bytes - (int64_t)r.stream_len;
    if (!ok) {
        if (lane < MPB_INFLATE_MSTAT) st[lane] = lane == 0 ? (uint32_t)MPB_BGZF_WHY_HEADER : 0u;      // not taken
        return;
    }
    BiLane L[BI_STATES];
    uint32_t iterations = 0;
    const uint32_t why = bi_member(in, r.stream_off, (uint32_t)r.stream_len, (uint32_t)r.out_len, (uint8_t *)s_window, &s_sh, L, lane,
                                   &iterations);
    if (why == BI_OK) bi_store_window(s_window, text, r.out_off, (uint32_t)r.out_len, lane);
    if (lane < MPB_INFLATE_MSTAT) {
        const uint32_t v = lane == 0 ? why : lane == 1 ? L[0].stored_blocks : lane == 2 ? L[0].fixed_blocks : lane == 3 ? L[0].dynamic_blocks
                         : lane == 4 ? L[0].literals : lane == 5 ? L[0].matches : lane == 6 ? L[0].matched_bytes : L[0].longest_code;
        st[lane] = v;
    }
}

}  // namespace

void mpb_launch_bgzf_inflate(const uint8_t *in, int64_t in_bytes, const mpb_bgzf_member_row *rows, int64_t n_members, uint8_t *text,
                             int64_t text_bytes, uint32_t *mstat, hipStream_t s)
{
    if (n_members <= 0) return;
    hipLaunchKernelGGL(k_bgzf_inflate, dim3((unsigned)n_members), dim3(BI_LANES), 0, s, in, in_bytes, rows, n_members, text, text_bytes,
                       mstat);
}
