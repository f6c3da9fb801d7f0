// mpb_hostonly.h -- the part of the C-ABI layer that needs no GPU (mpb_hostonly.cpp): error state, the table arithmetic, the
// packers, argument checks and the refusals several entries share, the narrow pass' cost model, the host Poisson tail, the NUMA
// parser, the environment's integers, what the inflating entries make of a BGZF member.  Includes no HIP header: the
// unit builds with a plain C++ compiler (tools/asan_api.sh, tools/tsan_poisson.sh run it under the host sanitizers).  C++
// linkage throughout, so the version script, which exports `mpb_*` only, keeps all of it inside the library.
#ifndef MPB_HOSTONLY_H
#define MPB_HOSTONLY_H

#include <sched.h>
#include <stddef.h>
#include "mpb_shared.h"

#define MPB_ERR_LEN 512                   // bytes of a thread's last error text (mpb_last_error)

// sets mpb_last_error() of the calling thread, returns code
int fail(int code, const char *fmt, ...);

static inline int64_t align_up(int64_t x, int64_t a) { return (x + a - 1) / a * a; }

struct MpbPair { double x, y; };          // one table entry; the layout of HIP's double2 (checked in mpb_ctx.h)
void lut_entry(int q, MpbPair *e, MpbPair *odds = nullptr);
void build_lut(MpbPair *lut, MpbPair *odds = nullptr);
int pack_one_read(const char *contig, const int32_t *quals, int32_t len, bool poisson, uint8_t *row, int32_t row_bytes,
                  MpbPair *h, bool *priv);

int check_params(const mpb_filter_params *p);
// the refusals several entries share, each with its one message (who: the entry's name as a prefix, or null)
const int64_t k_text_max_bytes = 1ll << 30;              // the text of one call, in every entry that takes text
int check_text_bytes(int64_t text_bytes);
int check_fastq_offset(int32_t fastq_offset, const char *who = nullptr);
// the integer in environment variable `name` when it lies in lo..hi, else (unset, empty, no number, out of range) `fallback`
int64_t env_int64(const char *name, int64_t lo, int64_t hi, int64_t fallback);
double inv_norm_cdf(double p);
// the parameters of a per-read call (bernoulli's calculate_errors_PB / calculate_errors_poisson): alpha, the rest moira's defaults
static inline mpb_filter_params per_read_params(double alpha)
{
    mpb_filter_params p;
    p.alpha = alpha; p.uncert = 1.0; p.maxerrors = NAN; p.ambig_mode = MPB_AMBIG_IGNORE; p.flags = 0;
    return p;
}

int narrow_rows_from_sample(const int32_t *hist, int n_sample, bool odds = false);
int64_t pipeline_chunk_reads(int64_t n, int64_t row_stride);
int poisson_finish_marked(const mpb_filter_params *p, const int32_t *ns, const int32_t *len, int32_t fixed_len, int64_t n,
                          double *ee, uint8_t *pass, int64_t *n_marked);

// CRC-32 of every BGZF member of a text (member m = bytes [m * MPB_BGZF_DATA, ...)), on a few threads
uint32_t bgzf_crc32(const uint8_t *p, size_t n);          // RFC 1952 section 8, eight bytes per step
void bgzf_member_crcs(const uint8_t *text, int64_t text_bytes, int64_t n_members, uint32_t *crc_out);
// What the inflating entries make of a member.  The reason of k_bgzf_inflate's status word (one the kernel never writes:
// MPB_BGZF_WHY_HEADER); a taken member's status row (eight words) added to the call's stats, longest_code as a maximum; and the one
// range [*lo, *hi) of `in` that holds the streams of the vouched-for rows (out_len >= 0) among n -- widening the range that is
// there when `any`, returning whether there is one now.
uint8_t bgzf_member_reason(uint32_t status_word);
void bgzf_stats_add(mpb_bgzf_inflate_stats *acc, const uint32_t *mstat_row);
bool bgzf_stream_range(const mpb_bgzf_member_row *rows, int64_t n, bool any, int64_t *lo, int64_t *hi);

bool parse_cpulist(const char *s, cpu_set_t *set, int *count);
int staging_threads();
void parallel_copy(void *dst, const void *src, size_t bytes, int threads);

#endif
