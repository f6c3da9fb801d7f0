// mpb_crc_kernels.hip -- RFC 1952's CRC-32 of ranges of a device text buffer (include/moira_pb.h, mpb_crc32_ranges_host /
// mpb_filter_bgzf_fastq_host): what lets text that k_bgzf_inflate wrote be trusted where it lies, without a round trip to the host.
//   k_bgzf_crc32   one wave per range {off, len} (len at most 65536: a BGZF member's text), four ranges per workgroup.  The
//                  workgroup first computes the four 256-entry tables of a slicing-by-four CRC into 4 KiB of LDS (32 shift
//                  steps per thread, one barrier).  Lane j then runs the table CRC over the j-th slice of 1024 bytes counted from
//                  the range's end, moves its register over the bytes behind the slice (one multiplication modulo the
//                  polynomial by a constant), and the wave's xor, inverted, is the CRC (mpb_crc_lane.inc: the identities).
// A lane reads only inside its slice -- bytes up to the first multiple of 16, aligned 16-byte words, bytes again -- and the range
// is checked against text_bytes here, whatever the host checked: a bad range gets crc 0 and the marker CRC_BAD_RANGE and reads
// nothing.  No workgroup waits for another; every loop runs over a slice or the 32 bits of a factor; results leave by plain
// vector stores.

#include "mpb_internal.h"

#define CRC_FN __device__ __forceinline__
#define CRC_CONST __device__ static const
typedef uint4 CrcWord;
#define CRC_LDW(text, p) (*reinterpret_cast<const uint4 *>((text) + (p)))
#define CRC_LDB(text, p) ((uint32_t)(text)[p])
#define CRC_TAB(tab, k, i) ((tab)[(k) * 256 + (i)])
#include "mpb_crc_lane.inc"

static_assert(CRC_LANES == 64 && CRC_RANGE_MAX == MPB_CRC_RANGE_MAX && sizeof(mpb_crc_range) == 16, "the CRC kernel's shapes");

#define CRC_WAVES 4                               // ranges per workgroup

namespace {

__global__ __launch_bounds__(CRC_WAVES * CRC_LANES) void k_bgzf_crc32(const uint8_t *__restrict__ text, int64_t text_bytes,
                                                                     const mpb_crc_range *__restrict__ ranges, int64_t n,
                                                                     uint32_t *__restrict__ crc, uint32_t *__restrict__ bad)
{
    __shared__ uint32_t s_tab[4 * 256];
    const int tid = (int)threadIdx.x;
    {
        uint32_t e[4];
        crc_table_entry((uint32_t)tid, e);
#pragma unroll
        for (int k = 0; k < 4; k++) s_tab[k * 256 + tid] = e[k];
    }
    __syncthreads();                                         // (the only one: before any wave leaves)
    const int j = tid & 63;
    const int64_t r = (int64_t)blockIdx.x * CRC_WAVES + (tid >> 6);
    if (r >= n) return;                                      // (wave-uniform, as is everything up to the slice loop)
    const mpb_crc_range g = ranges[r];
    if (!crc_range_ok(g.off, (int64_t)g.len, text_bytes)) {
        if (j == 0) { crc[r] = 0u; bad[r] = CRC_BAD_RANGE; }
        return;
    }
    CrcLane L;
    crc_lane_begin(g.off, (int64_t)g.len, j, &L);
    while (crc_lane_step(text, s_tab, &L)) { }
    uint32_t v = crc_lane_end(&L, j);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v ^= (uint32_t)__shfl_xor((int)v, d);
    if (j == 0) { crc[r] = v ^ 0xffffffffu; bad[r] = 0u; }
}

}  // namespace

void mpb_launch_bgzf_crc32(const uint8_t *text, int64_t text_bytes, const mpb_crc_range *ranges, int64_t n, uint32_t *crc,
                           uint32_t *bad, hipStream_t s)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_bgzf_crc32, dim3((unsigned)((n + CRC_WAVES - 1) / CRC_WAVES)), dim3(CRC_WAVES * CRC_LANES), 0, s, text,
                       text_bytes, ranges, n, crc, bad);
}
