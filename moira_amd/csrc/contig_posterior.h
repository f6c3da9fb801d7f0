// contig_posterior.h -- the two `posterior` consensus expressions of make_contig (moira/moira.py:1392-1396, :1520-1556), one libm
// pow / log10 chain each.  Included by contig.cpp (libmoira_contig.so: evaluated per column) and by mpb_hostonly.cpp
// (libmoira_pb.so: evaluated once per (q1, q2) into the two tables the device consensus reads -- there is no pow on the device).
// Both units are built with -ffp-contract=off, so both see the same IEEE operations in the same order.
#ifndef CONTIG_POSTERIOR_H
#define CONTIG_POSTERIOR_H

#include <cmath>

inline double qual2prob(int q) { return pow(10, q / (-10.0)); }                       // moira.py:1392-1393
inline int prob2qual(double p) { return (int)floor(-10 * log10(p)); }                 // moira.py:1395-1396

// the argument of prob2qual where both reads show the same base (:1520-1531) ...
inline double posterior_match_p(int fq, int rq)
{
    const double p1 = qual2prob(fq), p2 = qual2prob(rq);
    return (p1 * p2 / 3) / (1 - p1 - p2 + (4 * p1 * p2 / 3));
}
// ... and where they differ and fq != rq (:1533-1556): p1 belongs to the read with the higher quality, whose base wins
inline double posterior_mismatch_p(int fq, int rq)
{
    double p1, p2;
    if (fq > rq) { p1 = qual2prob(fq); p2 = qual2prob(rq); }
    else { p2 = qual2prob(fq); p1 = qual2prob(rq); }
    return p1 * (1 - p2 / 3) / (p1 + p2 - (4 * p1 * p2 / 3));
}

#endif
