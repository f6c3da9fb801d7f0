// mpb_bgzf_kernels.hip -- .gz output on the device (include/moira_pb.h, mpb_bgzf_compress_host): k_bgzf_deflate turns every
// BGZF member of a piece of text (at most MPB_BGZF_DATA bytes, its own window) into one complete raw-deflate stream, one workgroup
// of 256 lanes per member; k_bgzf_scan adds the members' sizes up (one block, as k_rag_scan does); k_bgzf_frame gathers header,
// stream and trailer of every member into the dense output.  What a lane does is mpb_bgzf_lane.inc (also compiled and checked on
// the host); here are the workgroup's own parts: the order of look-up and insertion, the scan of the token widths, the phases.
//
//   load    the member -> LDS, whole 32-bit words (the text's allocation is rounded up to 16 bytes); the hash table is cleared
//   match   steps of 256 positions in order: every lane looks its next 4 and its next 8 bytes up in the two tables, THEN (barrier)
//           every lane inserts with an LDS atomic max of position + 1 -- one winner, the largest position -- so a table entry
//           never depends on timing; both candidates and the distances 1..4 are verified byte by byte (bz_find)
//   parse   greedy, inside the same step: lane 0 walks the step's match lengths in LDS from the first uncovered position
//           (bz_walk_step) and marks the token starts; the token of every position (0: none) goes to the member's row of the
//           token array in global memory, the histograms to LDS (integer atomic adds)
//   code    lane 0: the three Huffman trees, the three costs, the choice (bz_plan_block)
//   emit    stored: header and text straight to the slot.  Otherwise the words of the bit buffer (the hash table's LDS, free
//           now) are cleared, lane 0 writes the block header while all lanes walk the tokens again, 256 positions per step: a
//           workgroup scan of the widths gives every token its bit offset, the bits go in with LDS atomic OR, and the words are
//           stored to the slot
// Every loop runs over the member's positions or a table of fixed size; no workgroup waits for another.
// LDS: 64 KiB text + 64 KiB hash table / bit buffer + the coder and the step arrays (about 137 KiB of the 160 KiB a gfx950
// workgroup may declare): one workgroup per CU.

#include "mpb_internal.h"

#define BZ_FN __device__ __forceinline__
#define BZ_LD8(text, i) ((text)[i])
__device__ __forceinline__ uint64_t bz_ld64_lds(const uint8_t *text, int i)
{
    uint64_t v;
    __builtin_memcpy(&v, text + i, 8);                       // (i + 8 <= MPB_BGZF_DATA + 8 <= the 65536 bytes of s_text)
    return v;
}
#define BZ_LD64(text, i, n) bz_ld64_lds((text), (i))
#define BZ_OR32(ptr, value) atomicOr((ptr), (value))
#include "mpb_bgzf_lane.inc"

static_assert(BZ_STEP == 256 && MPB_BGZF_DATA <= 65536 && MPB_BGZF_SLOT >= MPB_BGZF_DATA + 8, "k_bgzf_deflate's shapes");

namespace {

// exclusive prefix of v over the 256 lanes of the workgroup, and the total (s_wsum: 4 words of LDS; two barriers)
__device__ __forceinline__ uint32_t block_scan_256(uint32_t v, uint32_t *s_wsum, int tid, uint32_t *total)
{
    const int lane = tid & 63, wv = tid >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = (uint32_t)__shfl_up((int)inc, d);
        if (lane >= d) inc += o;
    }
    __syncthreads();                                         // (the previous step's readers of s_wsum are done)
    if (lane == 63) s_wsum[wv] = inc;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) { const uint32_t s = s_wsum[k]; all += s; if (k < wv) before += s; }
    *total = all;
    return before + inc - v;
}

__global__ __launch_bounds__(BZ_STEP) void k_bgzf_deflate(const uint8_t *__restrict__ text, int64_t text_bytes, int64_t n_members,
                                                           uint32_t *__restrict__ tok, uint8_t *__restrict__ slots,
                                                           uint32_t *__restrict__ size, uint32_t *__restrict__ mstat)
{
    __shared__ __align__(16) uint8_t s_text[65536];
    __shared__ __align__(16) uint32_t s_hash[BZ_HASH_SIZE];  // position + 1 per bucket; after the parse: the bit buffer
    __shared__ BzCoder s_cd;
    __shared__ uint16_t s_len[BZ_STEP];
    __shared__ uint8_t s_flag[BZ_STEP];
    __shared__ uint32_t s_wsum[4];
    __shared__ int s_cur;

    const int64_t m = blockIdx.x;
    if (m >= n_members) return;
    const int64_t off = m * (int64_t)MPB_BGZF_DATA;
    if (off >= text_bytes) return;
    const int n = (int)(text_bytes - off < (int64_t)MPB_BGZF_DATA ? text_bytes - off : (int64_t)MPB_BGZF_DATA);   // 1 .. 0xff00
    const int tid = (int)threadIdx.x;
    uint32_t *mtok = tok + m * (int64_t)MPB_BGZF_DATA;
    uint8_t *slot = slots + m * (int64_t)MPB_BGZF_SLOT;

    // load (off is a multiple of 256; the words that hold bytes [0, n) lie inside the allocation's 16-byte round-up)
    {
        const uint32_t *src = (const uint32_t *)(text + off);
        uint32_t *dst = (uint32_t *)s_text;
        const int nw = (n + 3) >> 2;
        for (int i = tid; i < nw; i += BZ_STEP) dst[i] = src[i];
        for (int i = tid; i < BZ_HASH_SIZE; i += BZ_STEP) s_hash[i] = 0;
        uint32_t *z = (uint32_t *)&s_cd;
        for (int i = tid; i < (int)((sizeof(uint32_t) * (BZ_NLL + BZ_ND + BZ_NCL)) / 4); i += BZ_STEP) z[i] = 0;   // the three histograms lead the struct
        if (tid == 0) { s_cur = 0; s_cd.n_lit = 0; s_cd.n_match = 0; s_cd.matched = 0; }
    }
    __syncthreads();

    // match + parse
    uint32_t my_lit = 0, my_match = 0, my_bytes = 0;
    for (int base = 0; base < n; base += BZ_STEP) {
        const int p = base + tid;
        const uint32_t ha = p < n ? bz_hash_a(s_text, n, p) : BZ_NO_HASH;
        const uint32_t hb = p < n ? bz_hash_b(s_text, n, p) : BZ_NO_HASH;
        const uint32_t cand_a = ha != BZ_NO_HASH ? s_hash[ha] : 0u;
        const uint32_t cand_b = hb != BZ_NO_HASH ? s_hash[hb] : 0u;
        __syncthreads();                                     // every look-up of the step before any insertion of it
        if (ha != BZ_NO_HASH) atomicMax(&s_hash[ha], (uint32_t)p + 1u);
        if (hb != BZ_NO_HASH) atomicMax(&s_hash[hb], (uint32_t)p + 1u);
        int len = 0, dist = 0;
        if (p < n) bz_find(s_text, n, p, cand_a, cand_b, &len, &dist);
        s_len[tid] = (uint16_t)len;
        s_flag[tid] = 0;
        __syncthreads();                                     // (also: the insertions before the next step's look-ups)
        if (tid == 0) s_cur = bz_walk_step(s_len, s_flag, base, n - base < BZ_STEP ? n - base : BZ_STEP, s_cur);
        __syncthreads();
        if (p < n) {
            uint32_t t = 0;
            if (s_flag[tid]) {
                if (len) {
                    int ls, le, lv, ds, de, dv;
                    bz_len_code(len, &ls, &le, &lv);
                    bz_dist_code(dist, &ds, &de, &dv);
                    t = bz_tok_match(len, dist);
                    atomicAdd(&s_cd.ll_freq[ls], 1u);
                    atomicAdd(&s_cd.d_freq[ds], 1u);
                    my_match++; my_bytes += (uint32_t)len;
                } else {
                    t = bz_tok_literal(s_text[p]);
                    atomicAdd(&s_cd.ll_freq[s_text[p]], 1u);
                    my_lit++;
                }
            }
            mtok[p] = t;
        }
    }
    atomicAdd(&s_cd.n_lit, my_lit); atomicAdd(&s_cd.n_match, my_match); atomicAdd(&s_cd.matched, my_bytes);
    __syncthreads();

    // code
    if (tid == 0) bz_plan_block(&s_cd, n);
    __syncthreads();
    const int btype = s_cd.btype;
    const uint32_t total_bits = s_cd.total_bits;
    uint32_t bytes;
    if (btype == BZ_STORED) {
        if (tid == 0) {
            slot[0] = 1; slot[1] = (uint8_t)(n & 0xff); slot[2] = (uint8_t)(n >> 8);
            slot[3] = (uint8_t)(~n & 0xff); slot[4] = (uint8_t)((~n >> 8) & 0xff);
        }
        for (int i = tid; i < n; i += BZ_STEP) slot[5 + i] = s_text[i];
        bytes = (uint32_t)n + 5u;
    } else {
        // emit: total_bits < 8 (n + 5), so the words used end inside the 16384 of the buffer and inside the slot
        uint32_t *words = s_hash;
        const int nw = (int)((total_bits + 31u) >> 5);
        for (int i = tid; i <= nw && i < BZ_HASH_SIZE; i += BZ_STEP) words[i] = 0;
        __syncthreads();
        if (tid == 0) bz_write_header(&s_cd, words);
        uint32_t bitbase = s_cd.hdr_bits;
        uint32_t t_next = tid < n ? mtok[tid] : 0u;          // (this lane's own stores of the parse; fetched a step ahead)
        for (int base = 0; base < n; base += BZ_STEP) {
            const int p = base + tid;
            const uint32_t t = t_next;
            t_next = p + BZ_STEP < n ? mtok[p + BZ_STEP] : 0u;
            const uint32_t w = (uint32_t)bz_token_bits(&s_cd, t);
            uint32_t step_bits;
            const uint32_t at = block_scan_256(w, s_wsum, tid, &step_bits);
            if (t && bitbase + at + w <= total_bits) bz_emit_token(&s_cd, words, bitbase + at, t);
            bitbase += step_bits;
        }
        if (tid == 0 && bitbase + s_cd.ll_len[BZ_EOB] <= total_bits) bz_put(words, bitbase, s_cd.ll_code[BZ_EOB], s_cd.ll_len[BZ_EOB]);
        __syncthreads();
        uint32_t *out = (uint32_t *)slot;
        for (int i = tid; i < nw; i += BZ_STEP) out[i] = words[i];
        bytes = (total_bits + 7u) >> 3;
    }
    if (tid == 0) {
        size[m] = bytes;
        uint32_t *st = mstat + m * 4;
        st[0] = (uint32_t)btype; st[1] = s_cd.n_lit; st[2] = s_cd.n_match; st[3] = s_cd.matched;
    }
}

// exclusive prefix of the members' framed sizes (size + 26: header 18, trailer 8), one block: off[0 .. n], off[n] = the bytes
// of the piece's output
__global__ __launch_bounds__(1024) void k_bgzf_scan(const uint32_t *__restrict__ size, int n, int64_t *__restrict__ off)
{
    __shared__ unsigned long long s_sum[1024];
    const int tid = threadIdx.x;
    const int per = (n + 1023) / 1024;
    const int a = min(n, tid * per), b = min(n, a + per);
    unsigned long long sum = 0;
    for (int k = a; k < b; k++) sum += (unsigned long long)size[k] + 26ull;
    s_sum[tid] = sum;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const unsigned long long x = tid >= o ? s_sum[tid - o] : 0;
        __syncthreads();
        s_sum[tid] += x;
        __syncthreads();
    }
    unsigned long long run = s_sum[tid] - sum;
    for (int k = a; k < b; k++) { off[k] = (int64_t)run; run += (unsigned long long)size[k] + 26ull; }
    if (tid == 1023) off[n] = (int64_t)s_sum[1023];
}

// one workgroup per member: the 18-byte BGZF header with BSIZE = size + 25, the deflate bytes of its slot, CRC-32 and ISIZE
__global__ __launch_bounds__(256) void k_bgzf_frame(const uint8_t *__restrict__ slots, const uint32_t *__restrict__ size,
                                                    const int64_t *__restrict__ off, const uint32_t *__restrict__ crc,
                                                    int64_t text_bytes, int64_t n_members, int64_t out_cap, uint8_t *__restrict__ out)
{
    const int64_t m = blockIdx.x;
    if (m >= n_members) return;
    const uint32_t sz = size[m];
    const int64_t at = off[m];
    if (sz > (uint32_t)MPB_BGZF_SLOT || at < 0 || at + (int64_t)sz + 26 > out_cap) return;      // (cannot happen; nothing is written outside out)
    const int64_t left = text_bytes - m * (int64_t)MPB_BGZF_DATA;
    const uint32_t isize = (uint32_t)(left < (int64_t)MPB_BGZF_DATA ? left : (int64_t)MPB_BGZF_DATA);
    uint8_t *dst = out + at;
    const uint8_t *src = slots + m * (int64_t)MPB_BGZF_SLOT;
    const int tid = (int)threadIdx.x;
    if (tid < 18) {
        const uint32_t bsize = sz + 25u;
        uint8_t b;
        switch (tid) {
        case 0: b = 0x1f; break; case 1: b = 0x8b; break; case 2: b = 8; break; case 3: b = 4; break;
        case 9: b = 0xff; break; case 10: b = 6; break; case 12: b = 'B'; break; case 13: b = 'C'; break; case 14: b = 2; break;
        case 16: b = (uint8_t)(bsize & 0xff); break; case 17: b = (uint8_t)(bsize >> 8); break;
        default: b = 0; break;
        }
        dst[tid] = b;
    } else if (tid < 26) {
        const int k = tid - 18;
        const uint32_t v = k < 4 ? crc[m] : isize;
        dst[18 + sz + k] = (uint8_t)(v >> (8 * (k & 3)));
    }
    for (uint32_t i = (uint32_t)tid; i < sz; i += 256u) dst[18 + i] = src[i];
}

}  // namespace

void mpb_launch_bgzf_deflate(const uint8_t *text, int64_t text_bytes, int64_t n_members, uint32_t *tok, uint8_t *slots,
                             uint32_t *size, uint32_t *mstat, hipStream_t s)
{
    if (n_members <= 0) return;
    hipLaunchKernelGGL(k_bgzf_deflate, dim3((unsigned)n_members), dim3(BZ_STEP), 0, s, text, text_bytes, n_members, tok, slots, size, mstat);
}

void mpb_launch_bgzf_scan(const uint32_t *size, int64_t n_members, int64_t *off, hipStream_t s)
{
    if (n_members <= 0) return;
    hipLaunchKernelGGL(k_bgzf_scan, dim3(1), dim3(1024), 0, s, size, (int)n_members, off);
}

void mpb_launch_bgzf_frame(const uint8_t *slots, const uint32_t *size, const int64_t *off, const uint32_t *crc, int64_t text_bytes,
                           int64_t n_members, int64_t out_cap, uint8_t *out, hipStream_t s)
{
    if (n_members <= 0) return;
    hipLaunchKernelGGL(k_bgzf_frame, dim3((unsigned)n_members), dim3(256), 0, s, slots, size, off, crc, text_bytes, n_members, out_cap, out);
}
