// mpb_pair_lane.inc -- what ONE LANE of the pairing step does (mpb_pair_kernels.hip: k_pair_rows, k_pair_count, k_pair_lists), with
// no wave intrinsic in it: a neighbour's count or a rank is an argument, so that a host program runs the same text with checked
// loads (tests/helpers/pair_lane_check.cpp).  The step stands between two device-written record indexes and k_contig's inputs:
// the validated pair descriptor, the header comparison, the LDS size class and the place in the class list.
// The includer has mpb_contig_args.h in front (cd_row_ok, cd_lds_bytes, MpbLdsClasses) and defines
//     PR_FN                        the function qualifier (__device__ __forceinline__ / static inline)
//     PR_LD_IDX(idx, k)            idx[k] of a record index of `rows` rows, asked for only when 0 <= k < 6 rows
//     PR_LDB(text, i)              byte i of a text, asked for only inside a header range pr_row / pr_hdr_range validated
// The checks are mpb_pair_rows' (mpb_hostonly.cpp), in its order, and the comparison is mio_first_header_mismatch's
// (csrc/fastio.cpp); those two are the yardsticks.  Every loop here runs over a header token or the class table.

#define PR_LANES 256                              // lanes of a workgroup of k_pair_count / k_pair_lists: one pair each
#define PR_WAVE  64
#define PR_CLASS_SLOTS 16                         // words of a workgroup's row of the count table (the classes, then zeros)

// The descriptor of pair i from row i of both indexes, by every check of mpb_pair_rows in its order but the rec_cap one (the
// call's rec_cap is the largest need + 8: that check cannot fail).  false: *o is a row cd_row_ok refuses (l1 = l2 = 0).
PR_FN bool pr_row(const int64_t *fidx, const int64_t *ridx, int64_t i, int64_t fbytes, int64_t rbytes, mpb_pair_row *o)
{
    o->fseq_off = 0; o->fqual_off = 0; o->fhdr_off = 0; o->rseq_off = 0; o->rqual_off = 0;
    o->l1 = 0; o->l2 = 0; o->hdr_len = 0; o->pad = 0;
    const int64_t ho = PR_LD_IDX(fidx, i * 6 + 0), hl = PR_LD_IDX(fidx, i * 6 + 1);
    const int64_t l1 = PR_LD_IDX(fidx, i * 6 + 3), l2 = PR_LD_IDX(ridx, i * 6 + 3);
    if (ho < 0 || hl < 0) return false;
    if (hl > fbytes || ho > fbytes - hl) return false;
    if (l1 < 0 || l2 < 0) return false;
    if (l1 > 0x7fffffffll || l2 > 0x7fffffffll || hl > 0x7fffffffll) return false;
    if (PR_LD_IDX(fidx, i * 6 + 5) != l1) return false;
    if (PR_LD_IDX(ridx, i * 6 + 5) != l2) return false;
    const int64_t fs = PR_LD_IDX(fidx, i * 6 + 2), fq = PR_LD_IDX(fidx, i * 6 + 4);
    const int64_t rs = PR_LD_IDX(ridx, i * 6 + 2), rq = PR_LD_IDX(ridx, i * 6 + 4);
    if (fs < 0 || fq < 0 || rs < 0 || rq < 0) return false;
    if (l1 > fbytes || fs > fbytes - l1) return false;
    if (fq > fbytes - l1) return false;
    if (l2 > rbytes || rs > rbytes - l2) return false;
    if (rq > rbytes - l2) return false;
    o->fseq_off = fs; o->fqual_off = fq; o->fhdr_off = ho; o->rseq_off = rs; o->rqual_off = rq;
    o->l1 = (int32_t)l1; o->l2 = (int32_t)l2; o->hdr_len = (int32_t)hl;
    return true;
}

// the header token of row i of an index, checked against its text (the reverse file's: pr_row looks at the forward one only)
PR_FN bool pr_hdr_range(const int64_t *idx, int64_t i, int64_t bytes, int64_t *off, int64_t *len)
{
    const int64_t ho = PR_LD_IDX(idx, i * 6 + 0), hl = PR_LD_IDX(idx, i * 6 + 1);
    *off = 0; *len = 0;
    if (ho < 0 || hl < 0 || hl > bytes || ho > bytes - hl) return false;
    *off = ho; *len = hl;
    return true;
}

// mio_first_header_mismatch's test of one pair: the lengths first, then the bytes; both ranges are validated
PR_FN bool pr_hdr_differs(const uint8_t *ftext, int64_t fho, int64_t fhl, const uint8_t *rtext, int64_t rho, int64_t rhl)
{
    if (fhl != rhl) return true;
    for (int64_t k = 0; k < fhl; k++)
        if (PR_LDB(ftext, fho + k) != PR_LDB(rtext, rho + k)) return true;
    return false;
}

// the size class of a validated descriptor: the first entry of the class table that holds cd_lds_bytes(l1, l2); -1 when cd_row_ok
// refuses the pair for a reason other than rec_cap (a length outside 1..MPB_CONTIG_MAX_LEN, the 16-bit score predicate), when no
// class holds it, or when the call takes no pair at all (take == 0: a fastq_offset or scores outside what the device takes)
PR_FN int pr_class(const mpb_pair_row &r, int64_t fbytes, int64_t rbytes, int maxabs, int take, const MpbLdsClasses &t)
{
    if (!take || !cd_row_ok(r, fbytes, rbytes, INT64_MAX, maxabs)) return -1;
    const int need = cd_lds_bytes(r.l1, r.l2);
    for (int k = 0; k < t.n && k < MPB_LDS_CLASS_MAX; k++)
        if (need <= t.cap[k]) return k;
    return -1;
}

// hdr_len + 2 (l1 + l2): the bytes of the pair's slot (rec_cap is the largest of them plus 8)
PR_FN int64_t pr_need(const mpb_pair_row &r) { return (int64_t)r.hdr_len + 2 * ((int64_t)r.l1 + r.l2); }

// A lane's rank among the lanes of its workgroup with the same class: the lanes below it in its wave (mine: the wave's ballot of
// class cls; lane: 0..63), after the whole waves below (wave_counts[w][PR_CLASS_SLOTS]: wave w's count per class)
PR_FN uint32_t pr_rank(unsigned long long mine, int lane, const uint32_t *wave_counts, int wave, int cls)
{
    const unsigned long long below = (1ull << lane) - 1ull;
    uint32_t rank = (uint32_t)__builtin_popcountll(mine & below);
    for (int w = 0; w < PR_LANES / PR_WAVE; w++)
        if (w < wave) rank += wave_counts[w * PR_CLASS_SLOTS + cls];
    return rank;
}

// where pair i goes: the class' first place, the pairs of the class in the workgroups before, the rank inside the workgroup
PR_FN int64_t pr_list_slot(uint32_t first, uint32_t before, uint32_t rank) { return (int64_t)first + before + rank; }
