// mpb_contig_kernels.hip -- k_contig: paired-read contigs on the device (include/moira_pb.h, mpb_contigs_text_host), one wave
// per pair.  What a lane does is mpb_contig_lane.inc (also compiled and checked on the host); here are the wave's own parts: the
// hand-over of the border cell between neighbouring lanes (one DPP wave_shr per step, as k_dp hands its boundary row on), the
// two wave maxima of the 3' fix-up, the prefix count of emitted columns, and the order of the phases.
//
//   load    both reads -> LDS (reverse complement, quality decode, range checks); a bad read hands the pair back
//   fill    l1 + nl - 1 steps, exactly; lane l owns C = ceil(l2 / 64) columns, its previous row stays in registers; 2-bit
//           pointers and the 16-bit scores of the last column and row go to LDS
//   fix-up  last-index maxima of the last column and row (two wave reductions)
//   trace   lane 0, at most l1 + l2 steps, one word per alignment column
//   contig  64 columns at a time: the consensus column, then the prefix count of the emitted ones
//   write   only now, when nothing can hand the pair back any more: slot, index row, the three numbers, done = 1
// Every LDS and global index derives from lengths cd_row_ok checked against the buffer sizes and rec_cap; a descriptor it
// refuses leaves done = 0 and touches nothing.  LDS is sized per launch (the host buckets the pairs by cd_lds_bytes).
// Also here: k_contig_rows, which turns done[] and the index written below into k_pack_text's row descriptors, so that the
// contigs can be filtered in the slots they were written to (mpb_contigs_filter_text_host; per pair: mpb_contig_rows.inc).

#include "mpb_internal.h"

#define CD_FN __device__ __forceinline__
__device__ __forceinline__ int cd_gload8(const uint8_t *p) { return *p; }
#include "mpb_contig_args.h"

#define CR_FN __device__ __forceinline__
__device__ __forceinline__ int cr_done(const uint8_t *done, int64_t i) { return done[i]; }
__device__ __forceinline__ int64_t cr_idx(const int64_t *out_idx, int64_t k) { return out_idx[k]; }
#include "mpb_contig_rows.inc"

namespace {

__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)v, m);
        v = o > v ? o : v;
    }
    return v;
}

template <int C>
__device__ void contig_pair(const MpbContigArgs &a, const mpb_pair_row &r, int64_t pi, uint8_t *lds, int lane)
{
    const CdShape sh = cd_shape(r.l1, r.l2);
    const CdLayout L = cd_layout(sh);
    int *hdr = (int *)(lds + L.hdr);
    uint32_t *col = (uint32_t *)(lds + L.col), *res = (uint32_t *)(lds + L.res);
    int16_t *lastcol = (int16_t *)(lds + L.lastcol), *lastrow = (int16_t *)(lds + L.lastrow);
    uint8_t *s1 = lds + L.s1, *s2 = lds + L.s2, *q1 = lds + L.q1, *q2 = lds + L.q2, *ptr = lds + L.ptr;

    const bool ok = cd_load_lane(r, a.ftext, a.rtext, a.prm.offset, lane, s1, s2, q1, q2);
    if (lane == 0) { lastcol[0] = 0; lastrow[0] = 0; }
    if (__ballot(!ok) != 0) return;                                  // (uniform) handed back
    __syncthreads();

    CdLane<C> st;
    cd_lane_init<C>(st, sh, s2, lane);
    int out = 0;
    const int steps = cd_fill_steps(sh);
    for (int t = 0; t < steps; t++) {
        // S(i, l * C) of lane l - 1's last step (wave_shr:1; lane 0 reads 0 through bound_ctrl: column 0)
        const int left_in = __builtin_amdgcn_update_dpp(0, out, 0x138, 0xf, 0xf, true);
        out = cd_fill_step<C>(st, sh, a.prm, lane, t, left_in, out, s1, ptr, lastcol, lastrow);
    }
    __syncthreads();

    const uint32_t ck = wave_max_u32(cd_scan_key(lastcol, sh.l1 + 1, lane));
    const uint32_t rk = wave_max_u32(cd_scan_key(lastrow, sh.l2 + 1, lane));
    int bci, bri;
    const int fix = cd_fixup(sh, ck, rk, &bci, &bri);
    if (lane == 0) cd_traceback<C>(sh, a.prm, s1, s2, ptr, lastcol, lastrow, fix, bci, bri, col, hdr);
    __syncthreads();
    const int K = hdr[0], score = hdr[1], fstart = hdr[2], fend = hdr[3], rstart = hdr[4], rend = hdr[5];
    if (K < 1 || K > sh.l1 + sh.l2) return;                          // the walk did not end: handed back
    if (a.aln_out && K > a.aln_cap) return;
    int ostart, oend; bool reversed;
    if (fstart < rstart) { ostart = rstart; oend = fend; reversed = false; }
    else { ostart = fstart; oend = rend; reversed = true; }

    const unsigned long long below = (1ull << lane) - 1ull;
    int clen = 0, gaps = 0, mism = 0;
    bool bad = false;
    for (int k0 = 0; k0 < K; k0 += CD_LANES) {
        const int k = k0 + lane;
        uint32_t v = 0;
        if (k < K) v = cd_column(a.prm, s1, s2, q1, q2, a.tab_match, a.tab_mism, col[K - 1 - k], k, ostart, oend, reversed);
        const unsigned long long em = __ballot((v & CD_EMIT) != 0);
        if (k < K) res[K - 1 - k] = v | ((uint32_t)(clen + __popcll(em & below)) << 20);
        clen += __popcll(em);
        gaps += __popcll(__ballot((v & CD_GAP) != 0));
        mism += __popcll(__ballot((v & CD_MISM) != 0));
        bad |= __ballot((v & CD_BAD) != 0) != 0;
    }
    if (bad) return;                                                 // a contig quality outside its byte: handed back
    __syncthreads();

    const int hl = r.hdr_len;
    uint8_t *slot = a.out_buf + pi * a.rec_cap;                      // hl + 2 clen <= hl + 2 (l1 + l2) <= rec_cap
    for (int k = lane; k < hl; k += CD_LANES) slot[k] = (uint8_t)cd_gload8(a.ftext + r.fhdr_off + k);
    for (int k = lane; k < K; k += CD_LANES) {
        const uint32_t v = res[K - 1 - k];
        if (v & CD_EMIT) {
            const int m = (int)(v >> 20);
            slot[hl + m] = (uint8_t)(v >> 4);
            slot[hl + clen + m] = (uint8_t)(v >> 12);
        }
        if (a.aln_out) {
            const uint32_t cv = col[K - 1 - k];
            const int i = (int)(cv & 0xffffu), j = (int)(cv >> 16);
            uint8_t *al = a.aln_out + pi * 2 * a.aln_cap;
            al[k] = i ? s1[i - 1] : (uint8_t)'-';
            al[a.aln_cap + k] = j ? s2[j - 1] : (uint8_t)'-';
        }
    }
    if (lane == 0) {
        int64_t *o = a.out_idx + pi * 6;
        const int64_t base = pi * a.rec_cap;
        o[0] = base; o[1] = hl; o[2] = base + hl; o[3] = clen; o[4] = base + hl + clen; o[5] = clen;
        a.overlap[pi] = oend - ostart; a.gaps[pi] = gaps; a.mism[pi] = mism;
        if (a.aln_out) { a.aln_len[pi] = K; a.score[pi] = score; }
        a.done[pi] = 1;
    }
}

__global__ __launch_bounds__(CD_LANES) void k_contig(const MpbContigArgs a)
{
    extern __shared__ __align__(16) uint8_t cd_lds[];
    const int64_t w = blockIdx.x;
    if (w >= a.count) return;
    const int64_t pi = a.list[w];
    if (pi < 0 || pi >= a.n) return;
    const mpb_pair_row r = a.rows[pi];
    if (!cd_row_ok(r, a.fbytes, a.rbytes, a.rec_cap, a.prm.maxabs)) return;
    if (cd_lds_bytes(r.l1, r.l2) > a.lds_cap) return;
    const int lane = (int)threadIdx.x;
    switch ((r.l2 + CD_LANES - 1) / CD_LANES) {
    case 1: contig_pair<1>(a, r, pi, cd_lds, lane); break;
    case 2: contig_pair<2>(a, r, pi, cd_lds, lane); break;
    case 3: contig_pair<3>(a, r, pi, cd_lds, lane); break;
    case 4: contig_pair<4>(a, r, pi, cd_lds, lane); break;
    case 5: contig_pair<5>(a, r, pi, cd_lds, lane); break;
    case 6: contig_pair<6>(a, r, pi, cd_lds, lane); break;
    default: break;
    }
}

// k_contig_rows: done[n] + the index k_contig wrote -> the row descriptors k_pack_text walks over the slot buffer, one thread per
// pair (mpb_contig_rows.inc).  It runs behind the k_contig launches on the same stream and reads what they wrote; rows[i] is
// written for every i < n, whatever the index holds.
__global__ __launch_bounds__(256) void k_contig_rows(const int64_t *__restrict__ out_idx, const uint8_t *__restrict__ done, int64_t n,
                                                     int64_t rec_cap, int32_t max_len, int64_t stride, mpb_text_row *__restrict__ rows)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    rows[i] = cr_row(out_idx, done, i, rec_cap, max_len, stride);
}

}  // namespace

void mpb_launch_contig_rows(const int64_t *out_idx, const uint8_t *done, int64_t n, int64_t rec_cap, int32_t max_len, int64_t stride,
                            mpb_text_row *rows, hipStream_t s)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_contig_rows, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, out_idx, done, n, rec_cap, max_len, stride, rows);
}

void mpb_launch_contigs(const MpbContigArgs &a, hipStream_t s)
{
    if (a.count <= 0 || a.lds_cap <= 0 || a.lds_cap > MPB_CONTIG_LDS_MAX) return;
    hipLaunchKernelGGL(k_contig, dim3((unsigned)a.count), dim3(CD_LANES), (size_t)a.lds_cap, s, a);
}
