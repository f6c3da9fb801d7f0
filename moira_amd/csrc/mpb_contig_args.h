// mpb_contig_args.h -- what mpb_contig.cpp hands k_contig (mpb_contig_kernels.hip).  The includer defines CD_FN and cd_gload8
// before it (see mpb_contig_lane.inc).  Not installed.
#ifndef MPB_CONTIG_ARGS_H
#define MPB_CONTIG_ARGS_H

#include <stdint.h>
#include "../../include/moira_pb.h"
#include "mpb_contig_lane.inc"

#define MPB_CONTIG_LDS_MAX 65536          // the largest dynamic LDS block a launch asks for

// The LDS size classes of a call, as a kernel takes them by value: cap[0 .. n) ascending (the table itself is k_lds_class[] of
// mpb_contig.cpp, which buckets on the host with it and hands it to k_pair_rows, which buckets on the device)
#define MPB_LDS_CLASS_MAX 16
struct MpbLdsClasses { int32_t cap[MPB_LDS_CLASS_MAX]; int32_t n; };

struct MpbContigArgs {
    const uint8_t *ftext; int64_t fbytes;                // capacity round_up(bytes, 16), zero past the text
    const uint8_t *rtext; int64_t rbytes;
    const mpb_pair_row *rows; int64_t n;                 // the descriptors of the whole chunk
    const int32_t *list; int64_t count;                  // this launch's pairs (positions in rows): one wave each
    int32_t lds_cap;                                     // bytes of LDS per wave of this launch
    CdParams prm;
    int64_t rec_cap;
    const int32_t *tab_match, *tab_mism;                 // posterior mode only
    uint8_t *out_buf; int64_t *out_idx; int32_t *overlap, *gaps, *mism; uint8_t *done;
    uint8_t *aln_out; int64_t aln_cap; int32_t *aln_len, *score;     // aln_out == nullptr: not asked for
};

#endif
