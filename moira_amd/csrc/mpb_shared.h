// mpb_shared.h -- what the kernels (mpb_kernels.hip), the GPU-facing host units and the HIP-free host unit (mpb_hostonly.cpp) share:
// the reference's verdict on one read and the few limits host-only code needs.  Includes no HIP header, so that a unit which
// includes only this builds with a plain C++ compiler; mpb_internal.h includes it behind <hip/hip_runtime.h>.
#ifndef MPB_SHARED_H
#define MPB_SHARED_H

#include <math.h>
#include <stdint.h>
#include "../../include/moira_pb.h"     // MPB_FLAG_*, MPB_AMBIG_*

#ifdef __host__                          // a HIP compile, or a C++ compile behind the HIP headers: what __forceinline__ stands for there
#define MPB_SHARED_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define MPB_SHARED_FN inline
#endif

// ---- the reference's verdict on one read (moira.py:827-831, 911, 925-926, 949-950) -------------------------------------------
// Shared by every kernel that finishes a read and by the host Poisson tail.  P is MpbDevParams or mpb_filter_params (the fields
// maxerrors, uncert, ambig_mode, flags).  Between mpb_add_ns and mpb_round_and_keep a caller may look at the ee (MPB_FLAG_FAST_FMA's
// "unsure" test); the helpers write no memory.
// the read's limit: --maxerrors if set, else len x --uncert (moira.py:925-926, 949-950)
template <typename P>
MPB_SHARED_FN double mpb_limit(const P &p, int li)
{
    return (p.maxerrors == p.maxerrors) ? p.maxerrors : (double)li * p.uncert;
}
// --ambigs treat_as_errors: the ambiguous bases (N and n) count as errors (moira.py:827-828)
template <typename P>
MPB_SHARED_FN double mpb_add_ns(const P &p, double e, int nsv)
{
    return p.ambig_mode == MPB_AMBIG_TREAT_AS_ERRORS ? e + (double)nsv : e;
}
// Rounds e IN PLACE -- --round floors the reported ee (moira.py:830-831) -- and returns whether the read is kept: e <= its limit,
// unless --ambigs disallow finds an upper-case 'N' in it (moira.py:911: 'n' does not count there, so has_n is the caller's,
// apart from the ambiguity count).  (The limit is computed here, after the disallow test: taking it precomputed as an argument
// costs k_serve four spilled registers.)
template <typename P>
MPB_SHARED_FN bool mpb_round_and_keep(const P &p, double &e, bool has_n, int li)
{
    if (p.flags & MPB_FLAG_ROUND) e = floor(e);
    if (p.ambig_mode == MPB_AMBIG_DISALLOW && has_n) return false;
    return e <= mpb_limit(p, li);
}

#define MPB_MAX_LEN 65535                 // longest read (perm_ns and the prepass' marker counts are 16 bits wide)

// the natural-order narrow pass (mpb_internal.h): the rows it can keep, and the buckets of the sample that picks them
#define MPB_NAR_MIN_ROWS 2
#define MPB_NAR_MAX_ROWS 4
#define MPB_NAR_BUCKETS 16                // k_sample: [0] reads with a lower-case 'n', [r] reads that need r rows (r = 1..14), [15] more

#endif
