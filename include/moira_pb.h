/*
 * moira_pb.h -- C ABI of libmoira_pb.so: the MI355X (gfx950) Poisson-binomial
 * read-quality filter.
 *
 * This is the drop-in boundary for ONE path of fpusan/moira: what
 * moira/bernoullimodule.c (the CPython-2 extension `bernoulli`) and
 * moira.py's per-read dispatch compute today.  Every entry point below names
 * the reference interface it replaces as `ref: file:line` (paths are relative
 * to the reference checkout).
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no C++/torch types.
 *   - Every function returns an int status: MPB_OK (0) or a negative MPB_E_*.
 *     mpb_last_error() returns a thread-local human-readable message for the
 *     last failing call on the calling thread.  Nothing throws across the ABI.
 *   - The caller owns every buffer it passes.  The context owns its device
 *     workspace, LUTs, stream and events and frees them in mpb_destroy().
 *   - One context per device; calls on one context must not overlap (one host
 *     thread per device, as moira's Pool workers were one process per task).
 *   - There is NO CPU implementation in this library.  If no HIP device is
 *     usable, mpb_create() fails with MPB_E_NODEVICE; nothing falls back.
 *
 * Quality-matrix encoding ("packed qscores"), produced by mpb_pack_read():
 *   one read = one row of `row_stride` bytes (row_stride % 16 == 0),
 *   byte k < len :  1..254  Phred score Q (Q==0 was clamped to 1,
 *                            ref: moira/bernoullimodule.c:104-107, moira/moira.py:814)
 *                   0        the base is 'N' (ambiguous; skipped by the DP,
 *                            ref: moira/bernoullimodule.c:196-199)
 *                   255      the base is 'n' (counted as ambiguous by the C
 *                            reference, ref: moira/bernoullimodule.c:196, but
 *                            not by `--ambigs disallow`, ref: moira/moira.py:911)
 *   byte k >= len:  ignored (the kernels mask it; 0 is conventional).
 */
#ifndef MOIRA_PB_H
#define MOIRA_PB_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* The library is built with -fvisibility=hidden: exactly the entry points declared in this header are exported. */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

#define MPB_OK            0
#define MPB_E_INVALID    -1   /* bad argument (ValueError on the Python side)   */
#define MPB_E_NODEVICE   -2   /* no usable HIP device / bad device id           */
#define MPB_E_HIP        -3   /* a HIP runtime call failed (message has detail) */
#define MPB_E_NOMEM      -4   /* device or host allocation failed               */
#define MPB_E_RANGE      -5   /* a qscore cannot be encoded (Q < 0; Q > 254 in a batch entry) */

/* --ambigs modes, ref: moira/moira.py:658-659, :827-828, :911 */
#define MPB_AMBIG_TREAT_AS_ERRORS 0
#define MPB_AMBIG_IGNORE          1
#define MPB_AMBIG_DISALLOW        2

/* flags for mpb_filter_params.flags */
#define MPB_FLAG_ROUND      1u   /* --round: floor(ee) before the compare, ref: moira/moira.py:830-831 */
#define MPB_FLAG_FAST_FMA   2u   /* contract a*v+b*w into one fma: 2 FP64 ops per cell instead of 3.  ee is then close to,
                                    not bit-identical with, the reference's: the interpolation divides by the mass of
                                    the crossing row, which is of order alpha, so the error grows like 1/alpha (worst
                                    relative difference over 3000 random reads: 6e-14 at alpha 0.005, 1.4e-10 at 1e-6,
                                    1e-7 at 1e-9).  The flag is therefore ACCEPTED ONLY FOR alpha >= 1e-5 (MPB_E_INVALID
                                    below), where ee stays within north_star's 1e-9 relative tolerance and the guard
                                    band below keeps every pass/fail flag EQUAL to the exact computation's: a read
                                    whose ee lands within 1e-9 relative of the threshold (or of an integer with
                                    MPB_FLAG_ROUND) is recomputed with the three-rounding arithmetic.  Off by default. */
#define MPB_FLAG_ODDS      128u  /* opt-in: the MAIN PASS of the sorted pipeline may run ONE fma per DP cell.  It factors
                                    prod (a_k + b_k x) = (prod a_k) * prod (1 + r_k x), r_k = p_k / (1 - p_k): the registers hold
                                    the coefficients w of the second product (w[j] += r_k * w[j-1], w[0] == 1), P0 = prod a_k is
                                    the reference's row 0 bit for bit, and row j of its table is P0 * w[j] (ODDS_MODE.md).
                                    Contract: ee within 1e-9 relative of the bit-exact result; ns identical; pass identical for
                                    every read; a read without a result (NaN) stays one.  The flag PERMITS the cheaper
                                    arithmetic, it never requires it: every read the mode cannot vouch for is recomputed by the
                                    three-rounding code, and mpb_filter_counts.n_overflow counts those reads too (as it does
                                    for MPB_FLAG_FAST_FMA).  They are: a read whose P0 is not >= 2^-900 (every w[j] <= 1 / P0,
                                    so above that nothing has overflowed; long reads of poor quality); a read whose ee lands
                                    within 1e-9 relative of its limit, or of an integer with MPB_FLAG_ROUND; a read whose CDF
                                    does not cross inside its class's rows; wide reads (more than 1024 rows); every read of a
                                    call that runs on a private table (scores above 254) or takes the one-read-per-wave path
                                    (mpb_filter_host: at most 4096 reads without MPB_FLAG_BATCHED_ONLY).  A call with the flag takes the sorted
                                    pipeline, never the narrow pass (unless MPB_FLAG_ODDS_NARROW is set too).  The error grows like 1/alpha, as MPB_FLAG_FAST_FMA's does
                                    (worst relative difference of a numpy model over 1500 reads of 300 bases: 1.4e-12 at alpha
                                    1e-4, 1.3e-11 at 1e-5, 1.0e-10 at 1e-6; at most 5e-13 on the golden sets at alpha 0.005 ..
                                    0.5), so the flag is ACCEPTED ONLY FOR alpha >= 1e-5 (MPB_E_INVALID below), a factor of
                                    about 70 under the contract.  Not together with MPB_FLAG_FAST_FMA (MPB_E_INVALID); combines
                                    with ROUND, DECISION_ONLY, COUNT_CELLS, TEST_UNDERPREDICT, NO_NARROW.  Off by default. */
#define MPB_FLAG_DECISION_ONLY 8u /* opt-in, NOT the reference's contract: a read whose expected errors are
                                    PROVABLY above the threshold (multiplicative Chernoff lower-tail bound on the
                                    Poisson-binomial quantile, from the prepass' mean) is reported pass = 0,
                                    ee = +infinity without running its DP.  The bound is taken BEFORE any DP runs, so it wins:
                                    a read it settles is +infinity whether or not its CDF would ever have crossed 1 - alpha.  A
                                    read it does not settle is computed exactly as usual, and there a NaN still means what it
                                    means without the flag: the CDF never crossed -- the reference's ReturnedNaNError.  Both
                                    are pass = 0, and every pass/fail flag equals the full computation's.  For
                                    pipelines that never look at the ee of a discarded read. */
#define MPB_FLAG_TEST_UNDERPREDICT 4u /* test hook: halve every predicted row budget so that the
                                         overflow (second) pass is exercised; results are unchanged */
#define MPB_FLAG_COUNT_CELLS 32u /* diagnostic (bench.py's fp64_valu.frac_algorithmic): mpb_filter_device also sums, over the reads
                                    its tile kernel reports, the DP cells the ALGORITHM needs -- sum_k min(k + 1, J) over a read's
                                    scored bases, J = rows up to and including the one whose CDF crosses 1 - alpha --
                                    as opposed to the cells its row-budget class pays for.  Fetched with
                                    mpb_last_algorithmic_cells().  Reads settled elsewhere (k_wide, MPB_FLAG_DECISION_ONLY) are
                                    not counted.  Results are unchanged. */
#define MPB_FLAG_BATCHED_ONLY 16u /* mpb_filter_host sends batches of <= 4096 reads through one launch with one
                                     read per wave (latency: what a per-read caller sees) instead of the sorted,
                                     tiled pipeline; this flag forces the pipeline.  Results are identical. */

#define MPB_FLAG_NO_NARROW 64u   /* never take the natural-order narrow pass (below): the call runs the sorted, tiled pipeline whatever
                                    the batch looks like.  For callers of the introspection entries that describe that pipeline
                                    (mpb_last_class_histogram, mpb_last_read_budgets, MPB_FLAG_COUNT_CELLS).  Results are identical. */
#define MPB_FLAG_NARROW_ROWS(r) (((uint32_t)(r) & 15u) << 8)   /* test / measurement hook: take the narrow pass with r rows (2..4)
                                    whatever the sample says and however small the batch; reads it cannot finish still go through the
                                    sorted pipeline, so results are identical. */

#define MPB_FLAG_NARROW_SPLIT(c) (((uint32_t)(c) & 255u) << 12)   /* test / measurement hook, with MPB_FLAG_NARROW_ROWS(r >= 3) on a
                                    ragged batch: groups of the pass whose longest read has at most c 16-byte chunks run with r - 1
                                    rows ("mixed rows"; the library picks c from its sample by itself).  Results are identical. */

#define MPB_FLAG_ODDS_NARROW (1u << 20)   /* opt-in, only together with MPB_FLAG_ODDS (alone: MPB_E_INVALID): mpb_filter_device may also
                                    take the natural-order narrow pass, which then runs the one-FMA arithmetic (a lane keeps P0 and
                                    w[1 .. R-1]; R operations per base instead of 3 R - 2).  Contract as MPB_FLAG_ODDS: ee within 1e-9
                                    relative, ns / pass / NaN identical, decisions exact.  The pass hands a read back to the sorted
                                    pipeline -- which runs it with MPB_FLAG_ODDS kept, so that n_overflow counts the ones the
                                    three-rounding code recomputes -- when its CDF does not cross inside the R rows; when its P0 is
                                    not >= 2^-900 (a lower-case 'n' makes it NaN); when its ee lies within 1e-9 * max(1, |ee|) of
                                    its limit, or of an integer with MPB_FLAG_ROUND; and, in a ragged batch, when its length lies
                                    outside its row.  No mixed rows in this form: MPB_FLAG_NARROW_SPLIT is ignored with the flag.
                                    Everything that keeps a call out of the narrow pass still does.  Off by default. */

#define MPB_FLAG_POISSON_DEVICE_TAIL (1u << 21)   /* opt-in, read by the Poisson HOST entries only (mpb_filter_poisson_host,
                                    mpb_filter_host_multi with poisson != 0; every other entry ignores the bit): the CDF tail of each
                                    chunk runs on the device behind k_lambda (k_poisson_tail, in place in the chunk's ee array), and
                                    the host tail runs only on the reads the kernel hands back.  Contract and hand-back rule: "the
                                    device tail" below, next to mpb_poisson_finish_device.  n_overflow = the reads the host
                                    finished, summed over the chunks.  alpha < 1e-5 with the flag is MPB_E_INVALID.  Off by default:
                                    without it the entries keep the reference's libm bits. */

/* kernel ids for mpb_kernel_time() */
#define MPB_K_PREPASS   0   /* lambda/sigma/Ns estimate + row classing        */
#define MPB_K_SCAN      1   /* class histogram scan / tile table              */
#define MPB_K_SCATTER   2   /* stable scatter of read indices by class        */
#define MPB_K_DP        3   /* the Poisson-binomial DP + epilogue (dominant)  */
#define MPB_K_OVERFLOW  4   /* re-run of reads whose predicted row count was too small */
#define MPB_K_LAMBDA    5   /* Poisson approximation: per-read sum of error probabilities */
#define MPB_K_WIDE      6   /* reads that need more than 1024 DP rows: one workgroup per read */
#define MPB_K_NARROW    7   /* natural-order narrow pass: one read per lane, 2..4 DP rows, the matrix read once */
#define MPB_K_FALLBACK  8   /* (rounds 5: the gather of the unfinished reads and the scatter of their results; unused since round 6: they run where they lie) */
#define MPB_K_SAMPLE    9   /* ... the batch sample that picks the pass */
#define MPB_K_POISSON_TAIL 10 /* Poisson approximation: the CDF tail on the device (percentile, +Ns / floor, predicate) */
#define MPB_K_PACK_TEXT 11   /* FASTQ text + record index -> the packed ragged matrix (k_pack_text) */
#define MPB_K_CONTIG    12   /* paired-read contigs: the launches of one chunk, one per size class (k_contig) */
#define MPB_K_CONTIG_ROWS 13 /* the device's contig index -> k_pack_text's row descriptors (k_contig_rows); also the four pairing
                              kernels of mpb_contigs_filter_fastq_host (k_pair_rows / _count / _scan / _lists) */
#define MPB_K_BGZF_DEFLATE 14 /* .gz output on the device: one raw-deflate stream per BGZF member (k_bgzf_deflate) */
#define MPB_K_BGZF_SCAN  15  /* ... the prefix of the members' sizes (k_bgzf_scan) */
#define MPB_K_BGZF_FRAME 16  /* ... header, stream and trailer of every member into the dense output (k_bgzf_frame) */
#define MPB_K_BGZF_INFLATE 17 /* BGZF .gz input on the device: one member per wave (k_bgzf_inflate) */
#define MPB_K_FQ_LINES  18   /* the FASTQ record index on the device: newlines and refusal flags per tile (k_fq_lines) */
#define MPB_K_FQ_SCAN   19   /* ... the prefix of the tiles' newlines (k_fq_scan) */
#define MPB_K_FQ_STARTS 20   /* ... the line starts (k_fq_starts) */
#define MPB_K_FQ_ROWS   21   /* ... one index row, kind and k_pack_text descriptor per record (k_fq_rows) */
#define MPB_K_COUNT     22

typedef struct mpb_ctx mpb_ctx;

/*
 * Filter parameters = the filter-relevant moira flags.
 *   alpha      --alpha     (0,1)   ref: moira/moira.py:668,736; moira/bernoullimodule.c:79-83
 *   uncert     --uncert    (0,1]   ref: moira/moira.py:663-665,949-950
 *   maxerrors  --maxerrors >0 or NaN when unset (then uncert mode)
 *                                  ref: moira/moira.py:666,925-926
 *   ambig_mode --ambigs            ref: moira/moira.py:658,827-828,911
 *   flags      MPB_FLAG_*
 */
typedef struct mpb_filter_params {
    double   alpha;
    double   uncert;
    double   maxerrors;
    int32_t  ambig_mode;
    uint32_t flags;
} mpb_filter_params;

/* Totals of one filter call (what moira prints at moira/moira.py:508-519). */
typedef struct mpb_filter_counts {
    int64_t n_reads;
    int64_t n_pass;
    int64_t n_fail;
    int64_t n_overflow;   /* reads the second pass re-ran: their CDF did not cross 1 - alpha inside the row budget of the main pass
                             (J > the class cap mpb_last_read_budgets reports; for a wide read, J > its predicted rows, which no
                             entry reports -- except where 1 - alpha == 1: every budget is then all of the read's rows), which
                             includes every read that has no result (NaN); with MPB_FLAG_FAST_FMA / MPB_FLAG_ODDS also the reads
                             those modes hand over.  Diagnostic. */
} mpb_filter_counts;

/* ---- library ------------------------------------------------------------ */
const char *mpb_version(void);
const char *mpb_last_error(void);
/* number of visible HIP devices (0 when there is none; never fails) */
int mpb_device_count(void);

/* ---- context ------------------------------------------------------------ */
/* Creates the per-device context: stream, events, the 256-entry {1-p, p'} LUT
 * built on the host with libm pow exactly as ref: moira/bernoullimodule.c:202
 * and :140-145 do, uploaded once. */
int mpb_create(int device_id, mpb_ctx **out);
int mpb_destroy(mpb_ctx *ctx);
/* The table itself, for pinning it in tests ("the LUT values themselves are part of the fixtures"):
 * a_out[q] = pow(1 - p, 1), b_out[q] = ((1-1+1)/(1.0*1)) * (p/(1-p)) * pow(1 - p, 1) with p = pow(10, q / -10.0),
 * ref: moira/bernoullimodule.c:202,140-145; entries 0 ('N') and 255 ('n') are the identity step {1, 0}.
 * mpb_host_lut computes it on the host exactly as mpb_create does (needs no device); mpb_device_lut reads back
 * what the context uploaded.  256 doubles each. */
int mpb_host_lut(double *a_out, double *b_out);
int mpb_device_lut(mpb_ctx *ctx, double *a_out, double *b_out);
/* The HIP stream the context launches on (as void*), for callers that want to
 * order their own work (e.g. torch) against it. */
int mpb_stream(mpb_ctx *ctx, void **stream_out);
int mpb_synchronize(mpb_ctx *ctx);

/* ---- device memory plumbing (so a ctypes-only host needs no torch) -------- */
int mpb_malloc(mpb_ctx *ctx, int64_t bytes, void **dptr_out);
int mpb_free(mpb_ctx *ctx, void *dptr);
int mpb_memcpy_h2d(mpb_ctx *ctx, void *dst_dev, const void *src_host, int64_t bytes);
int mpb_memcpy_d2h(mpb_ctx *ctx, void *dst_host, const void *src_dev, int64_t bytes);
int mpb_memset(mpb_ctx *ctx, void *dst_dev, int value, int64_t bytes);
/* Pinned (page-locked) host memory.  A batch handed to mpb_filter_host from such a buffer is DMA-ed where
 * it lies; one in ordinary pageable memory is first copied into the context's pinned staging blocks (by a few
 * threads, overlapped with the GPU work of the chunks before).  A parser that packs its reads straight into a
 * pinned matrix (ref: moira/moira.py:1177 builds one Python list per read instead) saves that copy.
 * mpb_host_free waits for the context's streams first. */
int mpb_host_alloc(mpb_ctx *ctx, int64_t bytes, void **hptr_out);
int mpb_host_free(mpb_ctx *ctx, void *hptr);

/* ---- packing (host, integer only) ---------------------------------------- */
/* Encode one read into a row of the quality matrix.
 * Replaces the list->int[] marshalling + Q0 clamp of
 * ref: moira/bernoullimodule.c:92-108 and the N test of :196.
 * `seq` may be NULL (no ambiguous bases).  Returns MPB_E_RANGE if a score is
 * negative (the Python reference raises ValueError, ref: moira/moira.py:1603-1604)
 * or above 254. Bytes [len, row_bytes) are zeroed. */
int mpb_pack_read(const char *seq, const int32_t *quals, int32_t len,
                  uint8_t *row_out, int32_t row_bytes);
/* Same from a raw FASTQ quality string (ASCII, `offset` = --fastq_offset,
 * ref: moira/moira.py:1177). */
int mpb_pack_read_ascii(const char *seq, const char *qual_ascii, int32_t len,
                        int32_t offset, uint8_t *row_out, int32_t row_bytes);

/* Batch form for a parser: n reads concatenated (read i = bytes [off[i], off[i+1]) of seq_cat and
 * qual_cat), FASTQ ASCII qualities, packed into n rows of row_stride bytes; at most `max_len`
 * bases of each read are kept (--truncate, ref: moira/moira.py:806-807; <= 0: no limit).
 * lens_out[i] = bases packed.  One C loop instead of one Python list per read
 * (ref: moira/moira.py:1177 builds `[ord(x) - offset for x in ...]` per read). */
int mpb_pack_batch_ascii(const char *seq_cat, const char *qual_cat, const int64_t *off, int64_t n,
                         int32_t fastq_offset, int32_t max_len, int64_t row_stride,
                         uint8_t *out, int32_t *lens_out);

/* On-device decode: raw ASCII quality bytes and base letters already in HBM
 * (two n x row_stride matrices) -> the packed quality matrix, elementwise, same rules as
 * mpb_pack_read_ascii.  d_err (device int32, may be NULL) counts bytes that decode to Q < 0 or
 * Q > 254 (those are written as Q1 / Q254). */
int mpb_decode_ascii_device(mpb_ctx *ctx, const uint8_t *d_seq, const uint8_t *d_qual_ascii, int64_t n,
                            int64_t row_stride, const int32_t *d_len, int32_t fixed_len,
                            int32_t fastq_offset, uint8_t *d_q_out, int32_t *d_err);

/* The inverse, for tests and benchmarks that need FASTQ-text matrices resident in HBM: packed byte 0 -> ('N', offset+2),
 * 255 -> ('n', offset+2), Q -> (one of ACGT, chr(Q + offset)).  mpb_decode_ascii_device of its output gives the packed
 * matrix back for every Q <= 255 - offset. */
int mpb_encode_ascii_device(mpb_ctx *ctx, const uint8_t *d_q, int64_t n, int64_t row_stride, int32_t fastq_offset,
                            uint8_t *d_seq_out, uint8_t *d_qual_out);

/*
 * Packing on the device from the text AS IT LIES IN THE FILE (one step further): a chunk of FASTQ text plus
 * its record index -- what include/moira_io.h's mio_fastq_index yields, and the shape mct_contigs_from_fastq gives its contigs
 * (include/moira_contig.h: out_buf + out_idx) -- becomes the packed, zero-padded ragged matrix, the lengths and the has-'N'
 * flags, with no host pack.  The bytes are those of moira_io.h's mio_pack, bit for bit.
 *
 * The index has six int64 columns per record.  This library does not include moira_io.h (the two libraries stay independent of
 * each other); the column numbers are restated here and must equal MIO_SEQ_OFF / MIO_QUAL_OFF / MIO_QUAL_LEN / MIO_IDX_COLS:
 */
#define MPB_IDX_SEQ_OFF  2   /* byte offset of the sequence line (stripped) */
#define MPB_IDX_QUAL_OFF 4   /* byte offset of the quality line (stripped) */
#define MPB_IDX_QUAL_LEN 5   /* its length = the bases of the record */
#define MPB_IDX_COLS     6

typedef struct mpb_text_row { int64_t seq_off, qual_off; int32_t len, pad; } mpb_text_row;   /* 24 bytes */

/*
 * Host only: the VALIDATED row descriptors of n records -- the only place offsets are trusted from.
 *   idx          int64[n_records][MPB_IDX_COLS]
 *   sel          NULL: rows 0..n-1 describe records 0..n-1 (n <= n_records); otherwise row k describes record sel[k]
 *   text_bytes   bytes of the text the offsets point into
 *   max_len      > 0: at most that many bases of each record are packed (mio_pack's rule: len = min(QUAL_LEN, max_len))
 *   row_stride   0: validation and *longest_out only (rows_out may be NULL), so that a caller can size the matrix first
 *   longest_out  the longest packed length (may be NULL)
 * Validation is never clamping.  MPB_E_INVALID with *bad_record = k (the position in sel order; bad_record may be NULL) when
 * an offset or a length is negative, seq_off + len or qual_off + len lies past text_bytes, sel[k] is outside 0..n_records-1,
 * a packed length is above 65535, or it is above a non-zero row_stride.  A record that ends exactly at text_bytes is fine.
 */
int mpb_text_rows(const int64_t *idx, int64_t n_records, const int64_t *sel, int64_t n, int64_t text_bytes,
                  int32_t max_len, int64_t row_stride, mpb_text_row *rows_out, int64_t *longest_out, int64_t *bad_record);

/*
 * k_pack_text: d_text + d_rows[n] (mpb_text_rows' descriptors, uploaded) -> d_q_out[n][row_stride] (row_stride % 16 == 0,
 * 16-byte aligned), d_len_out[n], d_flags_out[n] (bit 0: the packed part holds an upper-case 'N'; may be NULL).
 * Per base: Q = byte - fastq_offset, Q0 -> 1, sequence byte 'N' -> 0, 'n' -> 255 unless lower_n_is_base; bytes [len, row_stride)
 * are zero.  fastq_offset must lie in 0..255 (MPB_E_INVALID otherwise: every byte would be out of range).
 * d_text must be 16-byte aligned and its ALLOCATION must hold round_up(text_bytes, 16) bytes: the kernel fetches whole aligned
 * 16-byte words, never one outside [d_text, d_text + round_up(text_bytes, 16)), and no byte past a record's end reaches an output.
 * A quality below 0 or above 254 is written as Q1 / Q254 (as mpb_decode_ascii_device does) and reported through d_status, a
 * device int64[2] the CALLER initialises to INT64_MAX: [0] = the smallest row position k with some Q < 0, [1] = the same for
 * Q > 254 (atomic min).  mio_pack's answer from them: the first bad record is the smaller of the two, and its "positive values"
 * message wins when slot 0 holds that record.
 * A descriptor that mpb_text_rows would have refused (the kernel checks offsets and length against text_bytes and row_stride
 * again: nothing is read or written out of bounds whatever d_rows holds) gives a zero row and d_len_out[k] = -1, which
 * mpb_filter_device reports as a bad length.  Asynchronous on the context's stream.
 */
int mpb_pack_text_device(mpb_ctx *ctx, const uint8_t *d_text, int64_t text_bytes, const mpb_text_row *d_rows, int64_t n,
                         int32_t fastq_offset, int32_t lower_n_is_base, int64_t row_stride,
                         uint8_t *d_q_out, int32_t *d_len_out, uint8_t *d_flags_out, int64_t *d_status);

/* ---- the hot path --------------------------------------------------------- */
/*
 * Filter a batch that is RESIDENT IN HBM.
 *   d_q         device, n rows of row_stride bytes (row_stride % 16 == 0, 16-B aligned; a 64-B aligned
 *               matrix with row_stride % 64 == 0 is the fast layout: every 64-byte lane group then reads one
 *               sector -- a matrix offset by 16 bytes costs the prepass 7 %; and the narrow pass of batches of good reads
 *               then walks whole 128-byte lines at every row count, at other strides only with two rows; for RAGGED batches
 *               (d_len != NULL) make row_stride a multiple of 128: the narrow pass of ragged batches fetches, per read, only the
 *               lines its bases lie in, and a row that starts inside a line shares that line with its neighbour)
 *   d_len       device int32[n], or NULL when every read has `fixed_len` bases
 *   outputs     device: d_ee double[n], d_ns int32[n], d_pass uint8[n]
 *   counts      host, may be NULL (when non-NULL the call synchronises)
 * Per read i this computes what
 *   bernoulli.calculate_errors_PB(seq, quals, alpha)   ref: moira/bernoullimodule.c:66-114,182-263
 *   + process_data's "ee += Ns" / floor                ref: moira/moira.py:827-831
 *   + write_results' keep/discard predicate            ref: moira/moira.py:911,925-926,949-950
 * compute, with the Python semantics where the C reference has undefined
 * behaviour (first CDF row already above 1-alpha -> ee = 0,
 * ref: moira/moira.py:1611,1629 vs moira/bernoullimodule.c:254).
 * d_ee[i] is the value process_data returns (after +Ns / floor).
 * A read whose summed CDF never exceeds 1 - alpha has no result: ee = NaN, pass = 0 (the reference never leaves its loop there;
 * moira.py:456,818 call it ReturnedNaNError).  That takes an alpha within a few ulp of 0 -- below 1.1e-16, 1 - alpha is exactly 1
 * and most reads are such reads; a read without a scored base is 0 (+Ns) at every alpha, as in the reference (moira.py:1631-1632).
 * Asynchronous on the context's stream unless `counts` is given -- with one exception since round 5: a batch that is eligible for
 * the narrow pass (mpb_path_info below: fixed-length or ragged rows of up to 4096 bytes, default table, none of the opt-in flags,
 * >= 262144 reads or MPB_FLAG_NARROW_ROWS) synchronises on the stream inside the call -- once per 64 calls of the same batch shape
 * for the sample that picks the pass, and after every narrow pass for the 4-byte count of the reads it hands to the sorted
 * pipeline (the sub-batch is sized from it).  Callers that queue steps behind each other and must not stall pass
 * MPB_FLAG_NO_NARROW.
 *
 * Read length: up to 65535 bases (row_stride <= 65536; rounds 1-3: 16383).  A read whose DP needs at most 1024 rows --
 * every read of up to 1023 bases, and any longer read with fewer than about a thousand expected errors -- runs in one wave
 * (the running probability vector in registers, 16 rows per lane); one that needs more is run by a workgroup of up to
 * 16 waves, the row that crosses a wave boundary travelling through an LDS stream.  Same arithmetic either way.
 * What a read may NEED is 16384 DP rows (16 waves x 1024: about 16,000 expected errors).  A read of up to 16383 bases can
 * never need more; a longer one that does -- tens of thousands of bases of which a third are wrong -- gets ee = NaN, pass = 0.
 * (The reference's C extension keeps its table on the stack and overruns it near 1000 bases; its Python twin,
 * ref: moira/moira.py:1561-1634, has no limit -- `--error_calc poisson_binomial_py`.)
 *
 * A length in d_len outside 0..min(row_stride, 65535) is NEVER clamped: that read gets ee = NaN, pass = 0, Ns = 0 (so
 * a caller that passes counts == NULL and never synchronises on an error cannot consume a result computed on a
 * different length), a device-side counter is raised, and the next call on this context that fetches `counts` from
 * mpb_filter_device fails with MPB_E_INVALID and clears it.
 */
int mpb_filter_device(mpb_ctx *ctx,
                      const uint8_t *d_q, int64_t n, int64_t row_stride,
                      const int32_t *d_len, int32_t fixed_len,
                      const mpb_filter_params *params,
                      double *d_ee, int32_t *d_ns, uint8_t *d_pass,
                      mpb_filter_counts *counts);

/*
 * Classified at source.  For a batch that is PRODUCED on the device -- raw FASTQ text (ref:
 * moira/moira.py:1177) already in HBM -- the pass that decodes it also classifies it: mpb_decode_classify_device
 * decodes d_seq / d_qual_ascii into the packed matrix d_q_out exactly as mpb_decode_ascii_device does AND, from the
 * bytes it holds in registers anyway, sums the row-budget prediction, counts the ambiguous bases (d_ns) and fills the
 * class histograms.  mpb_filter_device_classified, called next on the same context with the same batch, parameters and
 * result arrays, starts at the histogram scan: the packed matrix is read once (by the DP), not twice, which removes
 * the classification pass of mpb_filter_device (16 % of a 300-bp step).  Results are identical to
 * mpb_decode_ascii_device + mpb_filter_device.  Any other filter call on the context in between invalidates the
 * classification (mpb_filter_device_classified then fails with MPB_E_INVALID; nothing stale is ever consumed).
 * Both are asynchronous on the context's stream (unless `counts` is given).
 * Rows of up to 16384 bytes (the fused pass parks whole rows in LDS); longer text: mpb_decode_ascii_device + mpb_filter_device.
 */
int mpb_decode_classify_device(mpb_ctx *ctx, const uint8_t *d_seq, const uint8_t *d_qual_ascii, int64_t n,
                               int64_t row_stride, const int32_t *d_len, int32_t fixed_len, int32_t fastq_offset,
                               const mpb_filter_params *params, uint8_t *d_q_out,
                               double *d_ee, int32_t *d_ns, uint8_t *d_pass, int32_t *d_err);
int mpb_filter_device_classified(mpb_ctx *ctx,
                                 const uint8_t *d_q, int64_t n, int64_t row_stride,
                                 const int32_t *d_len, int32_t fixed_len,
                                 const mpb_filter_params *params,
                                 double *d_ee, int32_t *d_ns, uint8_t *d_pass,
                                 mpb_filter_counts *counts);

/*
 * Same for a batch in HOST memory; synchronous (results are in the caller's arrays on return).
 * Replaces the per-read Pool.apply_async dispatch + .get() barrier of ref: moira/moira.py:431-454
 * with a chunked, double-buffered pipeline: the batch is cut into chunks of <= 128 MiB of qualities
 * (at least four per batch where it is large enough) and the host-to-device copy of chunk k+1, the kernels
 * of chunk k and the device-to-host copy of chunk k-1 run concurrently on three streams through FOUR
 * pinned/device slots (about 0.55 GiB of device memory, and as much pinned host memory when the input is pageable).
 * Inputs in pinned memory (mpb_host_alloc) are copied by DMA from where they lie.
 * Batches of <= 4096 reads take one launch with one read per wave, the read's DP rows spread over the wave's lanes (what a
 * per-read caller needs is latency; MPB_FLAG_BATCHED_ONLY forces the batched pipeline); up to 1 MiB of input is read by that
 * kernel straight from the library's pinned block (one runtime call, no copies), and up to 256 reads report their completion
 * through a word per read in the same block instead of the runtime's completion signal: 27 us for one read.  Results are
 * identical either way.
 * Lengths are validated, never clamped: a len[i] < 0, > row_stride or > 65535 fails the call with
 * MPB_E_INVALID before anything is computed (mpb_filter_device, whose lengths live on the device, gives such a
 * read ee = NaN, pass = 0 and reports the condition from a device-side counter when `counts` is requested).
 */
int mpb_filter_host(mpb_ctx *ctx,
                    const uint8_t *q, int64_t n, int64_t row_stride,
                    const int32_t *len, int32_t fixed_len,
                    const mpb_filter_params *params,
                    double *ee, int32_t *ns, uint8_t *pass,
                    mpb_filter_counts *counts);

/*
 * Text in, results out: a chunk of FASTQ text in HOST memory with its record index (see mpb_text_rows) is uploaded once,
 * packed on the device (k_pack_text) and filtered there; synchronous.  In this order: mpb_text_rows on the host, before
 * anything is uploaded (MPB_E_INVALID, *bad_record); row stride = round_up(max(longest, 1), 128), the ragged narrow pass'
 * layout; the text is uploaded whole (more than 1 GiB of text is MPB_E_INVALID: split the chunk); the descriptors are
 * uploaded; then consecutive row ranges whose piece of the matrix is at most 256 MiB are packed and filtered one after the
 * other -- mpb_filter_device (poisson == 0), or what mpb_filter_poisson_host computes (poisson != 0: k_lambda and the host
 * tail; with MPB_FLAG_POISSON_DEVICE_TAIL, mpb_filter_poisson_device) -- and the results are copied out at the end.
 *   ee, ns, pass        as mpb_filter_host; len_out int32[n] and flags_out uint8[n] (bit 0: an upper-case 'N' among the packed
 *                       bases) may be NULL
 *   counts              may be NULL; the totals over all pieces
 * A quality character outside the encodable range gives MPB_E_RANGE with mio_pack's message ("Qualities must have positive
 * values." / "quality exceeds the encodable maximum 254") and *bad_record = the first such record in sel order, and then NO
 * result array is written for any read.  Results are bit-identical to mio_pack + mpb_filter_host / mpb_filter_poisson_host on
 * the same records.  The staging blocks belong to the context, grow on demand and are freed with it.
 * (Environment MPB_TEXT_PIECE_BYTES: a smaller piece limit, for tests of the piece loop.)
 */
int mpb_filter_text_host(mpb_ctx *ctx, const char *text, int64_t text_bytes, const int64_t *idx, int64_t n_records,
                         const int64_t *sel, int64_t n, int32_t fastq_offset, int32_t max_len, int32_t lower_n_is_base,
                         const mpb_filter_params *params, int32_t poisson,
                         double *ee, int32_t *ns, uint8_t *pass, int32_t *len_out, uint8_t *flags_out,
                         mpb_filter_counts *counts, int64_t *bad_record);

/*
 * The FASTQ record index on the device (opt-in; the default indexer stays mio_fastq_index of libmoira_io.so, which is the
 * yardstick and the only code that defines an error): a chunk of FASTQ TEXT ALONE, in host memory, is uploaded once and indexed
 * there -- newlines counted per tile, their prefix, the line starts, one row per record (csrc/mpb_index_kernels.hip).
 *   text, text_bytes   at most 1 GiB
 *   final              the text ends the file: an unterminated last line counts as a line
 *   max_records        at most that many records are indexed (>= 0)
 *   max_len            > 0: k_pack_text's descriptors pack at most that many bases of a record (mio_pack's rule)
 *   idx_out            int64[idx_cap_rows][MPB_IDX_COLS]: the six columns of mio_fastq_index's row
 *   n, consumed, bad_kind   what mio_fastq_index returns and stores; rows [0, n + (bad_kind ? 1 : 0)) of idx_out are written
 * WHEN THE DEVICE TAKES THE TEXT (*why == 0) these equal mio_fastq_index(text, text_bytes, final, max_records, ...)'s, bit for
 * bit.  When it does not, *why says so and NOTHING ELSE is defined; the caller indexes on the host:
 *   MPB_FQ_WHY_NON_ASCII   a byte >= 0x80        MPB_FQ_WHY_LONE_CR   a '\r' that no '\n' follows immediately
 *   MPB_FQ_WHY_LINE_TABLE  the line table of the counted lines would not fit (more than MPB_FQ_INDEX_MAX_BYTES, or no memory)
 *   MPB_FQ_WHY_ROW_CHECK   a line start the device wrote failed its check against the text (never expected)
 * The device refuses a superset of what the host calls MIO_E_UNSUPPORTED: it looks at every byte up to the last newline (of a
 * final text: every byte), also behind the first bad record or behind max_records, where the host would not look.  Bytes behind
 * the last newline of a non-final text are not looked at by either: a "\r" that ends a block of a CRLF file is no reason.  It
 * never returns an index the host would not return, and a problem in the text's content never fails the call.
 * Argument errors are MPB_E_INVALID: a NULL pointer, a negative size, more than 1 GiB of text, and an idx_cap_rows below
 * min(max_records, the text's lines / 4) + 1 -- known once the lines are counted; *n then holds that number of records, so that
 * a caller who guessed may ask again.  Device memory is sized from the counted lines (one small read-back after the scan),
 * never from the worst case of one line per byte.  Synchronous; the staging blocks belong to the context.
 */
#define MPB_FQ_WHY_TAKEN      0
#define MPB_FQ_WHY_NON_ASCII  1
#define MPB_FQ_WHY_LONE_CR    2
#define MPB_FQ_WHY_LINE_TABLE 3
#define MPB_FQ_WHY_ROW_CHECK  4
#define MPB_FQ_INDEX_MAX_BYTES (4ll << 30)
int mpb_fastq_index_host(mpb_ctx *ctx, const char *text, int64_t text_bytes, int32_t final, int64_t max_records, int32_t max_len,
                         int64_t *idx_out, int64_t idx_cap_rows, int64_t *n, int64_t *consumed, int32_t *bad_kind, int32_t *why);

/*
 * Text alone in, index and results out: mpb_fastq_index_host's index and mpb_filter_text_host's filter from ONE upload.  In this
 * order: the text is uploaded; the index is built on the device; {n, first bad record, longest packed length} are read back; the
 * matrix is laid out at round_up(max(longest, 1), 128); records 0..n-1 are packed and filtered piece by piece from the
 * device-written descriptors (mpb_filter_text_host's piece loop, MPB_TEXT_PIECE_BYTES included); the results and the index are
 * copied back.  ee, ns, pass, len_out, flags_out hold idx_cap_rows entries (len_out and flags_out may be NULL); counts and
 * bad_record may be NULL.  *why != 0: handed back as above, and nothing was filtered.  Otherwise n, consumed, bad_kind and the
 * rows are mio_fastq_index's and the results are bit-identical to mio_fastq_index + mpb_filter_text_host on the same text;
 * MPB_E_RANGE with mio_pack's message and *bad_record are as there, and a record longer than 65535 packed bases is MPB_E_INVALID.
 */
int mpb_filter_fastq_host(mpb_ctx *ctx, const char *text, int64_t text_bytes, int32_t final, int64_t max_records, int32_t max_len,
                          int64_t *idx_out, int64_t idx_cap_rows, int64_t *n, int64_t *consumed, int32_t *bad_kind, int32_t *why,
                          int32_t fastq_offset, int32_t lower_n_is_base, const mpb_filter_params *params, int32_t poisson,
                          double *ee, int32_t *ns, uint8_t *pass, int32_t *len_out, uint8_t *flags_out,
                          mpb_filter_counts *counts, int64_t *bad_record);

/*
 * fasta+qual input on the device (opt-in; the default stays mio_fasta_qual_index of libmoira_io.so, which is the yardstick and the
 * only code that defines an error): a chunk of FASTA TEXT and a chunk of QUAL TEXT, in host memory, are uploaded once.  Both go
 * through the record index's line kernels (newlines per tile, their prefix, the line starts); record r is lines 2 r and 2 r + 1
 * of each, and the record stage (k_fa_count, k_fa_scan, k_fa_write; csrc/mpb_fasta_qual_kernels.hip) builds the buffer of slots
 * `header token | sequence | one byte per quality` and the six-column index over it.
 *   ftext / qtext      each at most 1 GiB           final, max_records, max_len     as mpb_fastq_index_host's, for both texts
 *   out, out_cap       the slots (at most 1 GiB); records are taken while their slots end at or before out_cap
 *   idx_out            int64[idx_cap_rows][MPB_IDX_COLS], offsets relative to out
 * WHEN THE DEVICE TAKES THE TEXTS (*why == 0): *n, *f_consumed, *q_consumed, *out_used, out[0, *out_used) and rows [0, *n) of
 * idx_out equal mio_fasta_qual_index(ftext, ..., qtext, ..., final, max_records, out, out_cap, ...)'s, bit for bit.  The
 * candidate records are min(max_records, lines of ftext / 2, lines of qtext / 2) (an unterminated last line counts only when
 * final); *n is the candidates that fit out_cap.
 * WHEN IT DOES NOT, *why says why, *which the text (0 fasta, 1 qual), *bad_record the first offending record where there is one
 * (else -1), and NOTHING ELSE is defined; the caller runs the host function.  MPB_FQ_WHY_NON_ASCII / LONE_CR / LINE_TABLE /
 * ROW_CHECK as above, and
 *   MPB_FA_WHY_NAMES      the header tokens of a record differ         MPB_FA_WHY_EMPTY   an empty sequence or quality line
 *   MPB_FA_WHY_TOKEN      a quality line that is not 1-3 digit tokens of at most 254 with single blanks or tabs between them
 *   MPB_FA_WHY_LENGTH     the tokens of a quality line are not as many as the bases
 *   MPB_FA_WHY_TRUNCATED  final, fewer than max_records candidates, and a text has lines left over
 * All or nothing: one such record among the candidates hands the whole call back, as the host returns MIO_E_UNSUPPORTED for the
 * whole call.  The device looks at every candidate, also behind the last that fits, and does not take a token of more than three
 * digits ("0007", which the host reads): it refuses a superset of what the host refuses, never takes texts the host would not,
 * and never returns anything the host would not return.  A problem in the texts' content never fails the call.
 * Argument errors are MPB_E_INVALID, said with or without a device: a NULL pointer, a negative size, a text or out_cap above
 * 1 GiB, and an idx_cap_rows below the candidates -- known once the lines are counted; *n then holds their number, so that a
 * caller who guessed may ask again.  Device memory is sized from the counted lines (one small read-back after the scan).  The
 * three kernels have no MPB_K_* id: they are timed under MPB_K_FQ_ROWS.  Synchronous; the staging blocks belong to the context
 * (the record index's two), so this call ends a resident generation as mpb_fastq_index_host does.
 */
#define MPB_FA_WHY_NAMES     5
#define MPB_FA_WHY_EMPTY     6
#define MPB_FA_WHY_TOKEN     7
#define MPB_FA_WHY_LENGTH    8
#define MPB_FA_WHY_TRUNCATED 9
int mpb_fasta_qual_index_host(mpb_ctx *ctx, const char *ftext, int64_t ftext_bytes, const char *qtext, int64_t qtext_bytes, int32_t final,
                              int64_t max_records, int32_t max_len, uint8_t *out, int64_t out_cap, int64_t *idx_out, int64_t idx_cap_rows,
                              int64_t *n, int64_t *f_consumed, int64_t *q_consumed, int64_t *out_used, int32_t *why, int32_t *which,
                              int64_t *bad_record);

/*
 * Two texts in, slots, index and results out: mpb_fasta_qual_index_host's buffer and mpb_filter_text_host's filter from ONE
 * upload.  {n, first record not taken, longest packed length} are read back; the matrix is laid out at
 * round_up(max(longest, 1), 128); records 0..n-1 are packed and filtered piece by piece from the device-written descriptors over
 * the slots with FASTQ offset 0 (mpb_filter_text_host's piece loop, MPB_TEXT_PIECE_BYTES included); results, index and slots are
 * copied back (out may be NULL here: no slots come back).  ee, ns, pass, len_out, flags_out hold idx_cap_rows entries (len_out,
 * flags_out, counts and bad_pack_record may be NULL).  *why != 0: handed back as above, and nothing was filtered.  Otherwise the
 * results are bit-identical to mio_fasta_qual_index + mpb_filter_text_host(fastq_offset = 0) on the same texts.  The slots and
 * their index stay on the device as the resident text of a new generation: mpb_format_text_host and mpb_collapse_text_host take
 * them by `resident`, exactly as after mpb_filter_fastq_host.
 */
int mpb_filter_fasta_qual_host(mpb_ctx *ctx, const char *ftext, int64_t ftext_bytes, const char *qtext, int64_t qtext_bytes, int32_t final,
                               int64_t max_records, int32_t max_len, uint8_t *out, int64_t out_cap, int64_t *idx_out,
                               int64_t idx_cap_rows, int64_t *n, int64_t *f_consumed, int64_t *q_consumed, int64_t *out_used,
                               int32_t *why, int32_t *which, int64_t *bad_record, int32_t lower_n_is_base,
                               const mpb_filter_params *params, int32_t poisson, double *ee, int32_t *ns, uint8_t *pass,
                               int32_t *len_out, uint8_t *flags_out, mpb_filter_counts *counts, int64_t *bad_pack_record);

/*
 * Paired-read contigs on the device (opt-in; the default builder stays mct_contigs_from_fastq of libmoira_contig.so): the
 * Needleman-Wunsch fill, the traceback and the consensus of a chunk of read pairs that are still FASTQ text, one wave per pair
 * (k_contig, csrc/mpb_contig_kernels.hip).  The contract is BYTE IDENTITY with mct_contigs_from_fastq on every pair the device
 * takes; a pair it does not take is HANDED BACK (done[i] = 0, nothing of slot i is defined) and the caller builds it with the
 * host aligner, so every data error is raised by the code that raises it today.  The device takes a pair when
 *   1 <= l1, l2 <= MPB_CONTIG_MAX_LEN;  (l1 + l2 + 2) * max(|match|, |mismatch|, |gap|) < 30000 (the CPU's 16-bit predicate);
 *   every base of the reverse read has a complement;  every quality byte - fastq_offset >= 0;  every contig quality q satisfies
 *   0 <= q + fastq_offset <= 255;  neither read holds a '-' (make_contig reads a '-' of the alignment as a gap);
 *   fastq_offset lies in 0..255 (otherwise the whole chunk is handed back).
 * One measured run (profiles/device_contig_rate.json): 65,536 pairs of 2 x 251 bases, 36.3 ms on 16 host threads, 21.0 ms through
 * this call, transfers included, none handed back.  No rate is promised; the path stays opt-in.
 */
#define MPB_CONTIG_MAX_LEN 384
typedef struct mpb_pair_row {            /* 56 bytes: offsets into the forward / reverse text */
    int64_t fseq_off, fqual_off, fhdr_off, rseq_off, rqual_off;
    int32_t l1, l2, hdr_len, pad;
} mpb_pair_row;
typedef struct mpb_contig_params {
    int32_t match, mismatch, gap, insert, deltaq, consensus /* 0 best, 1 sum, 2 posterior */, qscore_cap, trim_overlap;
} mpb_contig_params;

/*
 * Host only: the VALIDATED descriptors of n pairs from the two record indexes (the six columns of include/moira_io.h) -- the
 * only place the offsets are trusted from.  MPB_E_INVALID with *bad_record = i (may be NULL) when an offset or a length is
 * negative or lies past its text, a sequence and its quality line differ in length, a length is above 2^31 - 1, or
 * hdr_len + 2 (l1 + l2) > rec_cap.  Lengths the device does not take (0, above MPB_CONTIG_MAX_LEN) are NOT errors here.
 */
int mpb_pair_rows(const int64_t *fidx, const int64_t *ridx, int64_t n, int64_t ftext_bytes, int64_t rtext_bytes,
                  int64_t rec_cap, mpb_pair_row *rows_out, int64_t *bad_record);

/*
 * Host only: the two tables the device consensus reads in `posterior` mode, int32[256][256] each, indexed [forward q][reverse q]:
 * prob2qual of the reference's expression for two equal bases (match) and for two different ones of unequal quality (mismatch;
 * the diagonal is unused), with the host's libm -- the expressions contig.cpp evaluates (csrc/contig_posterior.h).  An entry
 * that is not a finite integer is INT32_MIN (such a column hands its pair back).
 */
int mpb_contig_posterior_tables(int32_t *match_out, int32_t *mismatch_out);

/*
 * The chunk call; synchronous.  In this order: mpb_pair_rows, before anything is uploaded (MPB_E_INVALID, *bad_record);
 * make_contig's parameter checks (insert > 0, deltaq > 0, qscore_cap >= 0, consensus 0..2: MPB_E_INVALID); both texts are
 * uploaded once, into allocations rounded up to 16 bytes and zeroed past the text; the pairs are bucketed by the LDS their
 * matrix needs and one launch is made per size class; the slots and arrays come back.  Slot i of out_buf (rec_cap bytes) and
 * row i of out_idx are written exactly as mct_contigs_from_fastq writes them: header token, contig, q + fastq_offset bytes.
 * done[i] = 1: the device built pair i; 0: handed back.  Optional (aln_out may be NULL): aln_out[i][0..1][aln_cap] receive
 * the two aligned strings (no terminator), aln_len_out[i] their length, score_out[i] the alignment score; a pair whose
 * alignment is longer than aln_cap is handed back.  n_done / n_handed_back (may be NULL) count.  n == 0 is MPB_OK.
 * The device blocks belong to the context and grow on demand.
 */
int mpb_contigs_text_host(mpb_ctx *ctx, const char *ftext, int64_t ftext_bytes, const int64_t *fidx,
                          const char *rtext, int64_t rtext_bytes, const int64_t *ridx, int64_t n, int32_t fastq_offset,
                          const mpb_contig_params *params, int64_t rec_cap,
                          char *out_buf, int64_t *out_idx, int32_t *overlap, int32_t *gaps, int32_t *mismatches, uint8_t *done,
                          char *aln_out, int64_t aln_cap, int32_t *aln_len_out, int32_t *score_out,
                          int64_t *n_done, int64_t *n_handed_back, int64_t *bad_record);

/*
 * The chunk call with the filter behind it (opt-in, beside the two calls it joins); synchronous.  Everything
 * mpb_contigs_text_host does, in its order and with its errors, up to and including the k_contig launches; then k_contig_rows
 * (one thread per pair, behind them on the context's stream, no synchronisation in between) turns done[] and the device's own
 * index into the row descriptors of k_pack_text -- a pair that was handed back is an empty read, and an index row is used only
 * when sequence and quality lengths agree, the packed length min(quality length, max_len if > 0) lies in 0..min(65535, stride)
 * and both lines lie inside the pair's own slot (otherwise {0, 0, -1}: k_pack_text's zero row of length -1; the kernel checks
 * every offset against the buffer once more); then mpb_filter_text_host's piece loop (pieces of at most 256 MiB,
 * MPB_TEXT_PIECE_BYTES, the three poisson forms, its order of errors) over the slot buffer where it lies; then all copies back.
 * The row stride is round_up(max(1, min(max over the listed pairs of l1 + l2, max_len if > 0)), 128): known before anything runs.
 *   filtered[i]         1 exactly for the pairs with done[i] = 1 of a chunk whose filter went through.  For them ee / ns / pass /
 *                       len_out / flags_out (the last two may be NULL) are what mpb_filter_text_host returns for the same slot
 *                       and index row; for every other pair the five values are undefined
 *   counts              may be NULL; the filtered pairs only (n_reads = their number)
 * A quality out of range in a contig, or a filter call that fails, does not fail the call: it returns MPB_OK with the contigs
 * complete, filtered all zero, *filter_rc and *filter_bad_record (may be NULL) what mpb_filter_text_host over the built pairs
 * would have returned (the record's position among them), and mpb_last_error() its message.  Errors of the contig parameters,
 * of mpb_pair_rows and of the filter parameters are returned before anything is uploaded.  A chunk of which the device takes no
 * pair returns as mpb_contigs_text_host does, filtered all zero.  MPB_FLAG_FAST_FMA, MPB_FLAG_ODDS and MPB_FLAG_ODDS_NARROW are
 * taken with mpb_filter_text_host's contract.
 */
int mpb_contigs_filter_text_host(mpb_ctx *ctx, const char *ftext, int64_t ftext_bytes, const int64_t *fidx,
                                 const char *rtext, int64_t rtext_bytes, const int64_t *ridx, int64_t n, int32_t fastq_offset,
                                 const mpb_contig_params *params, int64_t rec_cap,
                                 char *out_buf, int64_t *out_idx, int32_t *overlap, int32_t *gaps, int32_t *mismatches, uint8_t *done,
                                 char *aln_out, int64_t aln_cap, int32_t *aln_len_out, int32_t *score_out,
                                 int64_t *n_done, int64_t *n_handed_back, int64_t *bad_record,
                                 int32_t max_len, int32_t lower_n_is_base, const mpb_filter_params *filter_params, int32_t poisson,
                                 double *ee, int32_t *ns, uint8_t *pass, int32_t *len_out, uint8_t *flags_out, uint8_t *filtered,
                                 mpb_filter_counts *counts, int *filter_rc, int64_t *filter_bad_record);

/*
 * The chunk call with the filter behind it from the two mates' TEXT ALONE (opt-in): nothing is built on the host.  Both texts are
 * uploaded once and indexed on the device as mpb_fastq_index_host indexes one; the pairing step (csrc/mpb_pair_kernels.hip:
 * k_pair_rows, k_pair_count, k_pair_scan, k_pair_lists; what a lane does: csrc/mpb_pair_lane.inc) turns the two device-written
 * indexes into what the host builds today -- mio_first_header_mismatch's comparison, mpb_pair_rows' validated descriptors, the
 * LDS size classes and the class lists in pair order -- and mpb_contigs_filter_text_host runs from there, from its k_contig
 * launches on, in its order and with its errors.  k_contig reads the texts where the index kernels read them.
 *   ftext / rtext, ffinal / rfinal, max_records     as mpb_fastq_index_host's, per text (each at most 1 GiB)
 *   fidx_out, ridx_out        int64[idx_cap_rows][MPB_IDX_COLS]; rows [0, n_k + (k_bad_kind ? 1 : 0)) are written
 *   n_f, f_bad_kind, n_r, r_bad_kind     what mio_fastq_index(text_k, final_k, max_records) returns for each text
 *   n_pairs                   min(n_f, n_r)
 *   mismatch                  the first pair < n_pairs whose header tokens differ (mio_first_header_mismatch), or -1
 *   n_built                   mismatch < 0 ? n_pairs : mismatch: the pairs the chunk call runs over
 *   f_consumed, r_consumed    the first byte behind record n_pairs - 1 of each text: what mio_fastq_index(text_k, final_k, n_pairs)
 *                             consumes
 *   why, which                MPB_FQ_WHY_* as mpb_fastq_index_host's, and the text it speaks of (0 forward, 1 reverse; the forward
 *                             text is looked at first).  MPB_FQ_WHY_ROW_CHECK also when a device-written index row of a pair
 *                             < n_built fails one of mpb_pair_rows' checks (never expected).  *why != 0: NOTHING ELSE is defined
 *   rec_cap_out               the slot size the call chose: max over the n_built pairs of hdr_len + 2 (l1 + l2), plus 8
 *   out_buf[out_cap_bytes]    n_built slots of rec_cap bytes; every per-pair array (out_idx, overlap, gaps, mismatches, done, ee,
 *                             ns, pass, len_out, flags_out, filtered) holds idx_cap_rows entries, of which n_built are written
 * and max_len .. filter_bad_record are mpb_contigs_filter_text_host's.  There are no alignment strings and no contigs-only form.
 * CONTRACT, when *why == 0: the two indexes, n_f, n_r, the bad kinds and the consumed words equal the host indexer's; mismatch
 * equals mio_first_header_mismatch's over n_pairs pairs; and every other output is bit-identical to mpb_contigs_filter_text_host
 * on those two indexes cut to n_built rows with rec_cap = *rec_cap_out.  The device defines no error about content: a pair it does
 * not take is handed back (done = 0) exactly as there, and the caller builds it from the returned index rows.
 * Argument errors are MPB_E_INVALID and are said with or without a device; then make_contig's and the filter's parameter checks.
 * Two capacities are known only once the device has counted: an idx_cap_rows below min(max_records, lines / 4) + 1 of either text
 * is MPB_E_INVALID with the two needed record counts in *n_f / *n_r, and n_built * rec_cap > out_cap_bytes is MPB_E_INVALID with
 * *rec_cap_out and *n_pairs set (n_built <= n_pairs), so that a caller who guessed may ask again.
 * Timing: the four pairing kernels have no kernel id of their own (MPB_K_COUNT stays); they run inside MPB_K_CONTIG_ROWS' spans, as
 * k_bgzf_crc32 runs inside MPB_K_BGZF_INFLATE's.  Synchronous; the staging blocks belong to the context.
 */
int mpb_contigs_filter_fastq_host(mpb_ctx *ctx, const char *ftext, int64_t ftext_bytes, int32_t ffinal,
                                  const char *rtext, int64_t rtext_bytes, int32_t rfinal, int64_t max_records, int32_t fastq_offset,
                                  const mpb_contig_params *params, int64_t *fidx_out, int64_t *ridx_out, int64_t idx_cap_rows,
                                  int64_t *n_f, int32_t *f_bad_kind, int64_t *n_r, int32_t *r_bad_kind, int64_t *n_pairs,
                                  int64_t *mismatch, int64_t *n_built, int64_t *f_consumed, int64_t *r_consumed, int32_t *why,
                                  int32_t *which, int64_t *rec_cap_out, char *out_buf, int64_t out_cap_bytes, int64_t *out_idx,
                                  int32_t *overlap, int32_t *gaps, int32_t *mismatches, uint8_t *done, int64_t *n_done,
                                  int64_t *n_handed_back, int32_t max_len, int32_t lower_n_is_base,
                                  const mpb_filter_params *filter_params, int32_t poisson, double *ee, int32_t *ns, uint8_t *pass,
                                  int32_t *len_out, uint8_t *flags_out, uint8_t *filtered, mpb_filter_counts *counts, int *filter_rc,
                                  int64_t *filter_bad_record);

/*
 * .gz output on the device (opt-in; the default compressor stays the host's zlib).  The text is cut into BGZF members (SAM/BAM
 * specification section 4.1: gzip members that state their size in a 'B','C' extra field) of at most MPB_BGZF_DATA text bytes,
 * each its own window, and every member is compressed by one workgroup (k_bgzf_deflate, csrc/mpb_bgzf_kernels.hip): LZ77 with
 * a hash table in LDS (matches of 3..258 bytes at distances up to 32768, confined to the member; greedy parse), then whichever
 * of a dynamic-Huffman, a fixed-Huffman and a stored block is shortest.  The output is a function of the text alone: the same
 * text gives the same bytes on every call.  k_bgzf_scan and k_bgzf_frame put header (18 bytes, BSIZE = stream + 25), stream and
 * trailer (CRC-32 and ISIZE; the CRC is computed on the host while the kernels run) of all members behind each other, and that
 * dense stream is what is copied back.
 *
 * mpb_bgzf_bound (host only): *out_cap = text_bytes + 31 * ceil(text_bytes / MPB_BGZF_DATA), every member stored.
 * mpb_bgzf_compress_host: the members of text[0 .. text_bytes) in order into out, WITHOUT the format's end marker (the writer
 * appends it when it closes the file); *out_bytes = their length.  out_cap must be at least the bound (MPB_E_INVALID otherwise,
 * as for a NULL out / out_bytes or a NULL text with text_bytes > 0).  text_bytes == 0 gives zero members and *out_bytes = 0.
 * stats (may be NULL) receives the counts of the call.  A call of more than 1024 members (65,280 KiB of text) is cut into pieces
 * of 1024 members inside the call (environment MPB_BGZF_PIECE_MEMBERS: fewer, 1 .. 1024, for tests of the piece loop); per piece
 * the device holds about 447 MiB (text, 4 bytes of token per text byte, the slots, the framed output).  The blocks belong to
 * the context and grow on demand.  Synchronous.
 */
#define MPB_BGZF_DATA 0xff00
typedef struct mpb_bgzf_stats {
    int64_t members, dynamic, fixed, stored;       /* members = dynamic + fixed + stored: the block type each member got */
    int64_t literals, matches, matched_bytes;      /* tokens over all members; literals + matched_bytes = text_bytes */
} mpb_bgzf_stats;
int mpb_bgzf_bound(int64_t text_bytes, int64_t *out_cap);
int mpb_bgzf_compress_host(mpb_ctx *ctx, const char *text, int64_t text_bytes, uint8_t *out, int64_t out_cap,
                           int64_t *out_bytes, mpb_bgzf_stats *stats);

/*
 * BGZF .gz input on the device (opt-in; the default inflater stays the host's, libmoira_io's mio_bgzf_inflate_mt, which is also
 * the only code that defines an error).  BGZF members are independent and at most 64 KiB each way, so every member is inflated by
 * one wave (k_bgzf_inflate, csrc/mpb_inflate_kernels.hip): its whole text in LDS, the compressed bytes staged through a small LDS
 * ring, the Huffman tables built by the lanes together.  The device takes a SUBSET of what the host decoder takes: a member it
 * does not take is handed back (done[k] = 0, why[k] says where it stopped) and the caller inflates that member on the host.
 *
 * mpb_bgzf_member_rows (host only, no context): the VALIDATED row of every member -- the only place offsets are trusted from.
 * in[in_len] holds the members; offs / sizes / out_offs[n + 1] are the arrays mio_bgzf_scan fills (member k is in[offs[k],
 * offs[k] + sizes[k]), its text goes to bytes [out_offs[k], out_offs[k + 1]) of the output).  Per member the gzip header is parsed
 * here: magic, CM = 8, FLG = FEXTRA only, XLEN, the walk of the subfields to 'B','C' with a 2-byte value, BSIZE + 1 == sizes[k],
 * stream and trailer inside the member, ISIZE == out_offs[k + 1] - out_offs[k] and within 0 .. 65536.  rows_out[k] gets the
 * stream's place in `in`, the text's place in the output and both lengths, crc_out[k] the trailer's CRC-32.  A member that
 * cannot be vouched for gets out_len = -1 and why_out[k] = MPB_BGZF_WHY_HEADER (why_out may be NULL) -- never an error return.
 * MPB_E_INVALID is for the arguments: a NULL array, n or in_len negative, out_offs decreasing or starting below 0, a member
 * that does not lie inside in.
 *
 * mpb_bgzf_inflate_host: rows as above, then pieces of at most 4096 consecutive members (environment
 * MPB_BGZF_INFLATE_PIECE_MEMBERS: fewer, 1 .. 4096, for tests of the piece loop) whose compressed bytes are one contiguous range
 * of `in` of at most 4096 * 65536 bytes: that range and the rows are uploaded, k_bgzf_inflate runs, status, counters and the
 * piece's text range come back; then the CRC-32 of every taken member's text is computed on a few host threads and compared with
 * its trailer's.  done[k] = 1 only when the device took member k and CRC and length match; bytes of out that belong to a member
 * with done[k] = 0 are unspecified.  why (may be NULL) receives MPB_BGZF_WHY_* per member.  out_cap must be at least out_offs[n].
 * A problem in a member's content never fails the call.  stats (may be NULL) receives the counts of the call.  The device blocks
 * belong to the context and grow on demand (a piece of 4096 full members: 256 MiB each way).  Synchronous.
 */
#define MPB_BGZF_WHY_OK 0
#define MPB_BGZF_WHY_HEADER 1            /* mpb_bgzf_member_rows could not vouch for the member */
#define MPB_BGZF_WHY_BLOCK_TYPE 2        /* BTYPE 3 */
#define MPB_BGZF_WHY_STORED_LENGTH 3     /* LEN != ~NLEN */
#define MPB_BGZF_WHY_CODE_LENGTH_CODE 4  /* the code-length code is over-subscribed or incomplete, or a pattern without a code was met */
#define MPB_BGZF_WHY_REPEAT 5            /* repeat code 16 first, or a run past HLIT + HDIST */
#define MPB_BGZF_WHY_TREE 6              /* HLIT / HDIST too large, no end-of-block code, an over-subscribed or incomplete code */
#define MPB_BGZF_WHY_SYMBOL 7            /* a literal/length pattern without a code, or symbol 286 / 287 */
#define MPB_BGZF_WHY_DISTANCE 8          /* a distance pattern without a code, symbol 30 / 31, or a distance before the member's start */
#define MPB_BGZF_WHY_OVERRUN 9           /* more text than ISIZE */
#define MPB_BGZF_WHY_SHORT 10            /* the final block ended with less text than ISIZE */
#define MPB_BGZF_WHY_TRUNCATED 11        /* the stream ended inside a block */
#define MPB_BGZF_WHY_TRAILING_BYTES 12   /* bytes between the final block and the trailer */
#define MPB_BGZF_WHY_CRC 13              /* the text's CRC-32 is not the trailer's */
typedef struct mpb_bgzf_member_row { int64_t stream_off, out_off; int32_t stream_len, out_len; } mpb_bgzf_member_row;   /* 24 bytes */
typedef struct mpb_bgzf_inflate_stats {
    int64_t members, taken, handed_back;             /* members = taken + handed_back */
    int64_t stored_blocks, fixed_blocks, dynamic_blocks;   /* of the taken members, as are the counts below */
    int64_t literals, matches, matched_bytes;
    int64_t longest_code;                            /* the longest code length of any Huffman code built */
} mpb_bgzf_inflate_stats;
int mpb_bgzf_member_rows(const uint8_t *in, int64_t in_len, const int64_t *offs, const int32_t *sizes, const int64_t *out_offs,
                         int64_t n, mpb_bgzf_member_row *rows_out, uint32_t *crc_out, uint8_t *why_out);
int mpb_bgzf_inflate_host(mpb_ctx *ctx, const uint8_t *in, int64_t in_len, const int64_t *offs, const int32_t *sizes,
                          const int64_t *out_offs, int64_t n, uint8_t *out, int64_t out_cap, uint8_t *done, uint8_t *why,
                          mpb_bgzf_inflate_stats *stats);

/*
 * RFC 1952's CRC-32 on the device (k_bgzf_crc32, csrc/mpb_crc_kernels.hip): what lets text that the device inflated be trusted
 * where it lies.  mpb_crc32_ranges_host is the kernel's own entry -- one upload of text[text_bytes] (at most 1 GiB), the kernel,
 * one read-back: crc_out[k] = the CRC-32 of text[offs[k], offs[k] + lens[k]), equal to zlib's crc32, for n ranges of 0 .. 65536
 * bytes each at any offset; ranges may overlap, an empty range's CRC is 0.  Argument errors (said before the context is looked
 * at) are MPB_E_INVALID: a NULL pointer, n or text_bytes negative, a range that does not lie inside the text or is longer than
 * 65536 bytes (the message names the first such range).  n == 0 launches nothing.  The kernel has no MPB_K_* id of its own: its
 * launches are timed under MPB_K_BGZF_INFLATE, so after this call alone that slot holds the CRC kernel alone.  Synchronous.
 */
int mpb_crc32_ranges_host(mpb_ctx *ctx, const uint8_t *text, int64_t text_bytes, const int64_t *offs, const int32_t *lens, int64_t n,
                          uint32_t *crc_out);

/*
 * BGZF FASTQ filtered where it inflates: mpb_bgzf_inflate_host's members in, mpb_filter_fastq_host's results out, and the text
 * never crosses the link upwards.  The text of the call is `carry` (the partial record the previous call left; may be empty)
 * followed by the members' text: T = carry_len + out_offs[n_members] bytes, at most 1 GiB; out_offs[0] must be 0.  in, in_len,
 * offs, sizes, out_offs, n_members, done, member_why (may be NULL), stats (may be NULL) are mpb_bgzf_inflate_host's; everything
 * from `final` on, except text_out / text_cap, is mpb_filter_fastq_host's, with idx_out, consumed and bad_kind relative to the
 * call's text, carry included.  In this order: the arguments are checked (with or without a device); mpb_bgzf_member_rows
 * vouches for the members; the text is carved from the device index's stage; carry and the members' one contiguous range of
 * compressed bytes are uploaded; k_bgzf_inflate writes every member's text to its place behind the carry; k_bgzf_crc32 computes
 * the CRC-32 of every vouched-for member's range; status rows and CRC words come back.  done[k] = 1 only when the device took
 * member k and the CRC equals its trailer's; otherwise member_why[k] is its MPB_BGZF_WHY_* (MPB_BGZF_WHY_CRC: a mismatch).
 * ALL OR NOTHING: when any member has done = 0, *first_back is the lowest such member, *n = 0, no result and no text is written
 * and MPB_OK is returned -- the caller inflates the batch on the host and goes through mpb_filter_fastq_host, so every error in
 * a member's content stays the host decoder's.  When every member was taken (*first_back = -1) the index is built, the records
 * packed and filtered over the text where it lies, exactly as mpb_filter_fastq_host does from its upload (*why: the index's own
 * MPB_FQ_WHY_* refusals; MPB_E_RANGE and *bad_record as there), and text_out (may be NULL: no text comes back; else text_cap >= T)
 * receives the T bytes.  An idx_cap_rows that proves too small is MPB_E_INVALID with *n = the records, as there; asking again
 * repeats the whole call, inflation included.  k_bgzf_crc32 runs inside MPB_K_BGZF_INFLATE's timing span: after this call that
 * slot is inflate + CRC.  Synchronous; the staging blocks belong to the context.
 */
int mpb_filter_bgzf_fastq_host(mpb_ctx *ctx, const char *carry, int64_t carry_len, const uint8_t *in, int64_t in_len,
                               const int64_t *offs, const int32_t *sizes, const int64_t *out_offs, int64_t n_members, int32_t final,
                               int64_t max_records, int32_t max_len, uint8_t *text_out, int64_t text_cap, uint8_t *done,
                               uint8_t *member_why, int64_t *first_back, mpb_bgzf_inflate_stats *stats, int64_t *idx_out,
                               int64_t idx_cap_rows, int64_t *n, int64_t *consumed, int32_t *bad_kind, int32_t *why,
                               int32_t fastq_offset, int32_t lower_n_is_base, const mpb_filter_params *params, int32_t poisson,
                               double *ee, int32_t *ns, uint8_t *pass, int32_t *len_out, uint8_t *flags_out,
                               mpb_filter_counts *counts, int64_t *bad_record);

/*
 * Output records formatted on the device (k_fmt_count, k_fmt_scan, k_fmt_write; csrc/mpb_format_kernels.hip): records sel[k]
 * (sel NULL: k; any order, repeats allowed), k < nsel, of a text and its record index idx[n_records][MPB_IDX_COLS] become fasta
 * (kind 0), qual (1) or fastq (2) text, byte for byte what mio_format (include/moira_io.h) writes for the same arguments with
 * ee == NULL -- that function stays the definition of the output; its ";ee=...;" suffix is not offered here (it is
 * mpb_format_records_host's, below).  relabel (at most
 * 255 bytes) with relabel_index[nsel] (each >= 0) replaces the header token; labels[n_labels] (at most 16, each at most 255
 * bytes) with label_id[nsel] (-1: none) appends "\t" + label.
 * UPLOADED FORM (resident == 0): text[text_bytes] (at most 1 GiB) and idx go up once; any buffer and index of that layout do
 * (fastio.index's, or the contigs' out_buf + out_idx).  The selected rows are validated on the host first -- sel[k] in
 * 0..n_records-1, header, sequence and (kinds 1, 2) quality ranges inside the text, SEQ_LEN == QUAL_LEN for kinds 1 and 2,
 * relabel_index[k] >= 0, label_id[k] < n_labels -- and a bad one is MPB_E_INVALID with *bad_record = k before anything is
 * uploaded; the kernels make the same checks again.
 * RESIDENT FORM (resident != 0; text and idx NULL): the text and the device-written index that the last successful
 * mpb_filter_fastq_host, mpb_filter_bgzf_fastq_host or mpb_filter_fasta_qual_host call of this context left on the device are
 * read where they lie (for the
 * BGZF call: carry + members' text, as its index counts); n_records is that call's *n.  The context numbers these texts:
 * mpb_resident_text returns the generation in force (1, 2, ...), 0 for none.  Every successful call of these makes a new one.
 * THE CONTIG GENERATION.  mpb_contigs_filter_fastq_host drops the generation first, as listed below, and at its end keeps a new
 * one when *why == 0, *n_built > 0, *n_handed_back == 0 and the filter went through (*filter_rc == MPB_OK): the text is the slot
 * buffer (*n_built * rec_cap bytes), the index the device-written out_idx, n_records is *n_built, and the generation carries the
 * device's overlap, gaps and mismatches arrays as its aux (mpb_format_records_host's report lines).  In every other case the
 * generation stays none: all or nothing.  The slot block belongs to the contig stage: mpb_contigs_text_host and
 * mpb_contigs_filter_text_host may grow or overwrite it, so they set a generation THAT LIES IN THAT BLOCK to none, and only such a
 * one -- a single-end generation stays in force behind them.  mpb_contigs_filter_text_host itself leaves no generation.
 * The generation is set to none by every call that may move, grow, overwrite or free the blocks the text and index lie in,
 * whether it succeeds, fails or hands its text back: mpb_fastq_index_host, mpb_filter_fastq_host, mpb_filter_bgzf_fastq_host,
 * mpb_contigs_filter_fastq_host, mpb_fasta_qual_index_host, mpb_filter_fasta_qual_host and mpb_destroy.  No other call touches them.  A `resident` that is not the generation in force
 * is MPB_E_INVALID with a message that holds "is not resident", and nothing is touched.  Only sel, relabel_index, label_id and
 * the strings go up (the compressed form adds 16 bytes per member).  A device-written row that fails the kernel's check is never
 * expected: MPB_E_INVALID with *bad_record.
 * SIZES.  *text_needed receives the length of the formatted text once the scan has run.  Text form (bgzf == 0): an out_cap
 * below it is MPB_E_INVALID with *text_needed set, so a caller may ask again; else out[0, *out_bytes) is the text.  Compressed
 * form (bgzf != 0): out_cap must be at least mpb_bgzf_bound(*text_needed) (MPB_E_INVALID with *text_needed set otherwise); out
 * receives the BGZF members of the formatted text in order, without the end marker, byte for byte what mpb_bgzf_compress_host
 * returns for that text; stats (may be NULL) as there.  The formatted text is written in windows of at most 256 MiB
 * (environment MPB_FORMAT_PIECE_BYTES: less; the compressed form: whole members, at most MPB_BGZF_PIECE_MEMBERS' piece), each
 * copied back or compressed before the next; neither the text nor the members depend on the window.
 * Argument errors (said before the context is looked at) are MPB_E_INVALID: a NULL where a pointer is needed, a negative size,
 * kind outside 0..2, fastq_offset or out_offset outside 0..255, relabel without relabel_index, label_id without labels, more
 * than 16 labels or an over-long string, both or neither of text / idx and resident.  When a row fails, nothing is written.
 * The three kernels have no MPB_K_* id: they are timed under MPB_K_PACK_TEXT, so after this call alone that slot holds them
 * alone.  Synchronous; the staging blocks belong to the context.
 */
int mpb_format_text_host(mpb_ctx *ctx, const char *text, int64_t text_bytes, const int64_t *idx, int64_t n_records, int64_t resident,
                         const int64_t *sel, int64_t nsel, int32_t kind, int32_t fastq_offset, int32_t out_offset, int32_t clamp_q0,
                         int32_t max_len, const char *relabel, const int64_t *relabel_index, const char *const *labels,
                         int32_t n_labels, const int32_t *label_id, int32_t bgzf, uint8_t *out, int64_t out_cap, int64_t *out_bytes,
                         int64_t *text_needed, int64_t *bad_record, mpb_bgzf_stats *stats);
int64_t mpb_resident_text(mpb_ctx *ctx);

/*
 * mpb_format_text_host with the two pieces of the host formatter's per-record interface it leaves out; the same kernels, the
 * same two forms, windows, compressed form, *text_needed / ask-again convention and *bad_record.  mpb_format_text_host is this
 * call with ee and aux NULL and kind 4 refused.
 * ee (double[nsel], by POSITION k in sel; NULL: none): the USEARCH suffix ";ee=%.2f;size=1;" between the header token and the
 * label, exactly where mio_format(..., ee) places it, for kinds 0, 1, 2 and 4.  The device renders "%.2f" in 64-bit integers
 * from the bits of the double: the sign is the sign bit (-0.0 and -0.001 give "-0.00"); the magnitude m 2^-s becomes
 * q = round-half-even(100 m / 2^s) on the exact binary value and is printed as q / 100, '.', the two digits of q % 100 --
 * snprintf's result.  THE TAKEN DOMAIN is finite values with |ee| < 2^53.  Every ee[k] is checked on the host before anything is
 * uploaded: one outside the domain is MPB_E_INVALID with *bad_record = k and a message naming ee; the caller formats on the host
 * (the device defines no output for it).  The kernel makes the same check again.  ee always comes from the host, 8 bytes per
 * selected record, in either form.
 * kind 4 (MIO_FMT_REPORT; 3 is the collapse's names line and stays invalid): the contigs.report line of mio_format_report,
 * hdr[;ee=..;size=1;] "\t1\t" overlap "\t" gaps "\t" mismatches "\n" -- no leading mark, no label (labels and label_id must be NULL),
 * the header token ':' -> '_' or relabel + decimal.  The three numbers are aux[3 r .. 3 r + 2] of the RECORD r = sel[k], any
 * int32.  The sequence and quality columns of the row are neither read nor checked.  Uploaded form: aux is
 * int32[n_records][3] and required.  Resident form: aux must be NULL and the generation must be one that carries aux (the
 * contig generation, above); otherwise MPB_E_INVALID, with a message of its own (a generation in force that has no aux is
 * resident).  aux with any other kind is MPB_E_INVALID.
 */
int mpb_format_records_host(mpb_ctx *ctx, const char *text, int64_t text_bytes, const int64_t *idx, int64_t n_records, int64_t resident,
                            const int64_t *sel, int64_t nsel, int32_t kind, int32_t fastq_offset, int32_t out_offset, int32_t clamp_q0,
                            int32_t max_len, const char *relabel, const int64_t *relabel_index, const char *const *labels,
                            int32_t n_labels, const int32_t *label_id, const double *ee, const int32_t *aux, int32_t bgzf, uint8_t *out,
                            int64_t out_cap, int64_t *out_bytes, int64_t *text_needed, int64_t *bad_record, mpb_bgzf_stats *stats);

/*
 * The data-parallel part of the collapse of identical sequences, on the device (k_col_hash, k_col_group, k_col_rep;
 * csrc/mpb_collapse_kernels.hip).  For records k < n_records of a text and its record index idx[n_records][MPB_IDX_COLS] the
 * sequence is text[SEQ_OFF, SEQ_OFF + L), L = SEQ_LEN, or min(SEQ_LEN, max_len) when max_len > 0 -- mio_collapse_add's.
 *   hash[k]   uint64: what mio_py2_hash (include/moira_io.h) returns for that sequence, the CPython-2.7 string hash
 *   rep[k]    int32: the smallest k' <= k whose sequence has the same bytes (k itself for the first of its kind)
 * Both are what mio_collapse_add_grouped takes; neither depends on how the device schedules its lanes.
 * UPLOADED FORM (resident == 0): text[text_bytes] (at most 1 GiB) and idx go up once; any buffer and index of that layout do.
 * The rows are validated on the host first -- the sequence's offset and length non-negative, the range inside the text -- and a
 * bad one is MPB_E_INVALID with *bad_record = k before anything is uploaded; the kernel makes the same check again.
 * RESIDENT FORM (resident != 0; text and idx NULL): the text and the device-written index that the last successful
 * mpb_filter_fastq_host or mpb_filter_bgzf_fastq_host call of this context left on the device are read where they lie;
 * n_records is that call's *n; the generations are mpb_format_text_host's (above), and so is what ends one.  A `resident` that
 * is not the generation in force is MPB_E_INVALID with a message that holds "is not resident", and nothing is touched.  This
 * call does not end the generation: a format call and a collapse call may follow each other on it in either order.  A
 * device-written row that fails the kernel's check is never expected: MPB_E_INVALID with *bad_record.
 * Argument errors (said before the context is looked at) are MPB_E_INVALID: a NULL where a pointer is needed (bad_record;
 * hash and rep when n_records > 0), a negative size or max_len, n_records above 2^31 - 1, both or neither of text / idx and
 * resident.  n_records == 0 succeeds and writes nothing.
 * The three kernels have no MPB_K_* id: they are timed under MPB_K_PACK_TEXT, as the formatter's.  Synchronous; the staging
 * block (hashes, 2^ceil(log2(2 n)) owner slots and their first records, the slot of every record) belongs to the context.
 */
int mpb_collapse_text_host(mpb_ctx *ctx, const char *text, int64_t text_bytes, const int64_t *idx, int64_t n_records,
                           int64_t resident, int32_t max_len, uint64_t *hash, int32_t *rep, int64_t *bad_record);

/*
 * The same batch call over SEVERAL contexts (normally one per GPU of the node) from one host process: the batch is
 * cut into n_ctx contiguous, balanced shards in read order, one host thread per context runs mpb_filter_host
 * (poisson == 0) or mpb_filter_poisson_host (poisson != 0) on its shard, and every shard's results land in the
 * caller's arrays at the shard's offset -- gathered in read order, no exchange step, no collective.
 * Replaces `Pool(args.processors)` of ref: moira/moira.py:398-399 for a host-fed caller: n_ctx PCIe links from one
 * process.  A context must not be listed twice.  counts (may be NULL) receives the totals over all shards.
 * On failure the status and message of the first failing shard are returned (other shards may have completed).
 */
/* The split mpb_filter_host_multi uses (and moira_amd/shard.py, for one process per GPU): rank r of `world` owns the
 * contiguous range [*lo, *hi) of n reads; the first n % world ranks get one read more.  Host-only. */
int mpb_shard_bounds(int64_t n, int32_t world, int32_t rank, int64_t *lo, int64_t *hi);
int mpb_filter_host_multi(mpb_ctx *const *ctxs, int32_t n_ctx,
                          const uint8_t *q, int64_t n, int64_t row_stride,
                          const int32_t *len, int32_t fixed_len,
                          const mpb_filter_params *params,
                          double *ee, int32_t *ns, uint8_t *pass,
                          mpb_filter_counts *counts, int32_t poisson);

/*
 * One read, the exact signature-level twin of
 *   bernoulli.calculate_errors_PB(contig, contig_quals, alpha) -> (ee, Ns)
 * ref: moira/bernoullimodule.c:66-114.  Validates alpha in (0,1) (:79-83),
 * clamps Q0->1 (:104-107), counts 'N' and 'n' (:196).  `ee` is the raw
 * percentile (no +Ns, no floor).  Runs the HIP path on a batch of one.
 * Any non-negative int is a valid score, as in the reference (:92-108): a read with scores above 254 -- which the byte
 * matrix of the batch entries cannot hold -- gets its own code table for the call ({1-p, p'} of every such score, by the
 * same expressions, under a byte code the read does not use).  MPB_E_RANGE only for a negative score, or for a read with
 * more than 254 distinct scores of which some exceed 254.
 * A stream of such calls pays no kernel launch each (round 5): while they come, the context keeps the one-read kernel
 * resident -- the call writes the packed read into a mailbox in pinned host memory and waits for the kernel's answer there.
 * That kernel leaves by itself 100 ms after its launch at the latest (so a context that is no longer called holds nothing
 * on the GPU), and before any call on this context frees memory.  Environment MPB_SERVE=0: a launch per call, as before.
 */
int mpb_calculate_errors_PB(mpb_ctx *ctx, const char *contig,
                            const int32_t *contig_quals, int32_t len,
                            double alpha, double *ee, int32_t *ns);

/* ---- batches with scores above 254 (round 4) ---------------------------------------------------------------------- */
/*
 * ref: moira/bernoullimodule.c:92-108 takes any int score; the byte matrix has 254 score codes.  mpb_pack_batch_coded packs a
 * batch (concatenated sequences -- NULL: no ambiguous bases -- and INTEGER scores, off[n + 1] offsets; max_len > 0 truncates,
 * moira/moira.py:806-807) and gives every distinct score above 254 a byte code the batch does not use, from 254 down;
 * code_scores[256] receives what each code stands for (code_scores[c] == c for the untouched ones; entries 0 and 255 are the
 * N / n markers).  MPB_E_RANGE when the batch has more such scores than free codes (split it, or use the per-read entry) or a
 * negative score.  mpb_filter_host_coded is mpb_filter_host on such a matrix: the call runs on a private copy of the
 * {1 - p, p'} table in which code c carries the values of score code_scores[c] (same libm expressions); NULL = the plain
 * entry.  A code should stand for a score >= its own value: the row predictor reads codes as scores, so a code that
 * understates its error probability only costs re-runs, never a result.  Poisson-binomial methods only.
 */
int mpb_pack_batch_coded(const char *seq_cat, const int32_t *qual_cat, const int64_t *off, int64_t n, int32_t max_len,
                         int64_t row_stride, uint8_t *q_out, int32_t *len_out, int32_t *code_scores);
int mpb_filter_host_coded(mpb_ctx *ctx, const uint8_t *q, int64_t n, int64_t row_stride, const int32_t *len,
                          int32_t fixed_len, const mpb_filter_params *params, const int32_t *code_scores,
                          double *ee, int32_t *ns, uint8_t *pass, mpb_filter_counts *counts);

/* ---- per-read calls from many worker processes: the broker -------------------------------------- */
/*
 * Reference shape: moira/moira.py:398-399,431-454 -- `Pool(args.processors)` worker processes, each calling
 * bernoulli.calculate_errors_PB(contig, contig_quals, alpha) once per read (moira/moira.py:817) and blocking for the
 * answer.  One GPU context per worker makes those one-read launches time-share the card.  Instead ONE process -- the
 * broker -- owns the GPU; the workers never touch it: mpb_broker_call() packs the read (host only, the packer of
 * mpb_calculate_errors_PB) into the caller's slot of a shared-memory segment and waits, the broker gathers whatever is
 * pending into one launch of the one-read-per-wave kernel (several such micro-batches in flight) and hands the results
 * back through the slots -- or (the default since round 5) keeps ONE kernel resident while calls arrive, a wave per slot that
 * polls the slot itself (the segment is registered with the runtime: the worker's row, parameters and door word are read
 * where they are written, the answer lands in the slot; MPB_BROKER_DIRECT=0: a mailbox of the broker's own copies): no
 * launch per call, and no pass through the broker thread; that kernel leaves by itself after 100 ms and is launched again
 * while calls keep coming (environment MPB_BROKER_SERVER=0: the launches).
 * Results are those of mpb_calculate_errors_PB bit for bit, scores above 254 included.
 *
 *   mpb_broker_serve   runs the broker loop on `ctx` in the calling thread until mpb_broker_shutdown(name), or until no
 *                      live process has been attached and nothing has been asked for idle_exit_ms milliseconds
 *                      (0: never).  Creates the segment "/moira_pb_<name>" (letters, digits, '_', '-', '.'), n_slots
 *                      (1..256) slots = the most worker processes it serves at once; replaces a segment a dead broker
 *                      left behind; MPB_E_INVALID when a live broker of that name exists.  Blocking.
 *   mpb_broker_attach  no ctx, no HIP call: maps the segment (waiting up to wait_ms for a broker that is still starting)
 *                      and claims a slot for this process.  An attachment does not survive fork(): the child attaches
 *                      itself (mpb_broker_call refuses an attachment made by another pid).
 *   mpb_broker_call    the per-read entry, arguments and errors of mpb_calculate_errors_PB.  MPB_E_HIP when the broker
 *                      stops or dies while the read is pending (the caller may start a new one and attach again).
 *   mpb_broker_stats   reads served / launches (micro-batches, or generations of the resident kernel) / reads run alone (row budget missed, or scores above
 *                      254), the broker's pid (0: not serving) and the number of attached processes; any may be NULL.
 */
typedef struct mpb_broker_client mpb_broker_client;
int mpb_broker_serve(mpb_ctx *ctx, const char *name, int32_t n_slots, int32_t idle_exit_ms);
int mpb_broker_attach(const char *name, int32_t wait_ms, mpb_broker_client **client_out);
int mpb_broker_call(mpb_broker_client *client, const char *contig, const int32_t *contig_quals, int32_t len,
                    double alpha, double *ee, int32_t *ns);
int mpb_broker_detach(mpb_broker_client *client);
int mpb_broker_shutdown(const char *name);
int mpb_broker_stats(const char *name, int64_t *served, int64_t *batches, int64_t *solo, int32_t *pid, int32_t *attached);

/* NUMA placement (round 5).  Each shard thread of mpb_filter_host_multi restricts itself, before its pipeline starts, to the
 * CPUs of the NUMA node its GPU hangs off -- /sys/bus/pci/devices/<bus id>/numa_node, /sys/devices/system/node/node<k>/cpulist,
 * intersected with what the process may use -- so that the pinned staging blocks it allocates and first touches, and the threads
 * that copy a pageable input into them, are node-local (8 GPUs fed from one socket do not scale).  No NUMA information, or
 * MOIRA_PB_NO_NUMA in the environment: threads stay where they are.  mpb_numa_cpulist_for_pci is that lookup, host-only
 * (sysfs_root "" or NULL = the real tree; a directory holding a copy of the two files for tests): *node_out = the node or -1,
 * cpulist_out = its CPU list as sysfs prints it ("0-47,96-143"). */
int mpb_numa_cpulist_for_pci(const char *sysfs_root, const char *pci_bus_id, int32_t *node_out, char *cpulist_out, int32_t cpulist_len);

/* ---- --error_calc poisson -------------------------------------- */
/*
 * Poisson approximation, ref: moira/moira.py:1637-1679 (calculate_errors_poisson).
 * Device part (a pure streaming reduction, the one variant that is HBM-bound):
 *   d_lambda[i] = sum over non-'N' bases, IN BASE ORDER, of pow(10, q / -10.0) (host-built LUT),
 *   bit-identical to the reference's sequential `Lambda += 10**(qscore / -10.0)`; d_ns[i] = #'N'.
 * NOTE the Python reference treats only upper-case 'N' as ambiguous here (moira.py:1660); a
 * byte 255 ('n') is therefore rejected by this entry point -- pack such a base as a normal one.
 */
int mpb_poisson_lambda_device(mpb_ctx *ctx, const uint8_t *d_q, int64_t n, int64_t row_stride,
                              const int32_t *d_len, int32_t fixed_len,
                              double *d_lambda, int32_t *d_ns);
/*
 * Host tail, exactly the reference's scalar loop with the same libm calls (exp, pow) and the
 * correctly rounded factorials Python's int->float conversion yields: CDF until > 1-alpha,
 * interpolate, then +Ns / floor / predicate as for the Poisson-binomial path.  lambda/ns are host
 * arrays (e.g. copied back from mpb_poisson_lambda_device).  ee is NaN where the reference would
 * raise OverflowError (more than 170 terms or pow overflow).
 */
int mpb_poisson_finish_host(const double *lambda, const int32_t *ns, const int32_t *len,
                            int32_t fixed_len, int64_t n, const mpb_filter_params *params,
                            double *ee, uint8_t *pass);
/* Both steps for a batch in host memory, through the same chunked, overlapped pipeline as mpb_filter_host (the host tail
 * of a chunk runs while the GPU works on the next chunks).  Lengths may be as long as the row (no 1023-base limit here). */
int mpb_filter_poisson_host(mpb_ctx *ctx, const uint8_t *q, int64_t n, int64_t row_stride,
                            const int32_t *len, int32_t fixed_len, const mpb_filter_params *params,
                            double *ee, int32_t *ns, uint8_t *pass, mpb_filter_counts *counts);

/*
 * The device tail.  mpb_poisson_finish_host is the reference's loop with the HOST's libm (exp, and one pow per CDF term); no
 * device code can have those bits -- glibc's exp / pow are not correctly rounded and differ between its own FMA and non-FMA
 * variants.  The two entries below (and MPB_FLAG_POISSON_DEVICE_TAIL) therefore carry the contract of MPB_FLAG_FAST_FMA /
 * MPB_FLAG_ODDS, with mpb_poisson_finish_host as the exact side:
 *   - ee within 1e-9 relative; an ee of 0 on either side is 0 on both;
 *   - ns, every pass / fail flag and every NaN identical;
 *   - every read the device arithmetic cannot vouch for is finished by the host tail and counted in n_overflow.
 * Device arithmetic (k_poisson_tail, one read per lane): em = exp(-lambda), one call per read and no pow; the terms by
 * recurrence t_0 = em, t_j = (t_{j-1} * lambda) / j; the CDF summed sequentially until it exceeds 1 - alpha (j <= 170, as the
 * reference's factorial); the reference's interpolation (j - 1) + (thr - acc_prev) / (acc - acc_prev), negative -> 0; then +Ns /
 * floor / predicate by the code the host tail uses.
 * Hand-back rule -- a read goes to the host tail when
 *   (a) !(lambda >= 0 && lambda <= 64): NaN, negative, infinite, and every lambda for which the reference can raise OverflowError
 *       (lambda <= 64: lambda ** j <= 2^1020 for every j <= 170, and with alpha >= 1e-5 the CDF crosses long before term 170).
 *       Every read that can be NaN is computed by the code that defines it;
 *   (b) its CDF crosses in term 0 or 1 and |(1 - alpha) - em| < 2^-17: in term 1 the ee is the fraction (thr - em) / t_1 alone, so
 *       a last-bit difference in em is a large relative error once thr - em is tiny; in term 0 the two sides could disagree
 *       between 0 and a tiny positive value.  The window was fixed on a numpy model of this arithmetic with em moved by -1 / 0 / +1
 *       ulp against mpb_poisson_finish_host (tests/test_poisson_device_model.py).  Worst relative error of the model outside the
 *       window, per alpha -- over 100 k lambda uniform in [0, 64]: 1e-5: 1.1e-11, 1e-4: 1.2e-12, 0.005: 2.5e-13, 0.05: 5.7e-13,
 *       0.5: 9.0e-14, 0.9: 4.2e-13; over every input family of the tests (planted neighbours of the cancellation point, one-base
 *       reads): 1e-5: 1.8e-11, 1e-4: 7.3e-12, 0.005: 9.4e-12, 0.05: 7.7e-12 -- at least 50 x inside the contract; the crossing
 *       term and the ee == 0 reads agree everywhere outside the window;
 *   (c) its ee (after +Ns) lies within 1e-9 * max(1, |ee|) of its limit or, with MPB_FLAG_ROUND, of an integer -- the test of
 *       MPB_FLAG_FAST_FMA / MPB_FLAG_ODDS.  Not asked of a read that crosses in term 0 outside the window of (b): its ee is 0 (+Ns)
 *       exactly on both sides.
 * alpha < 1e-5 is MPB_E_INVALID (the floor of the other tolerance modes; the exact entries -- mpb_poisson_finish_host,
 * mpb_filter_poisson_host without the flag -- take any alpha).
 * BOTH ENTRIES SYNCHRONISE before they return: they fetch the 4-byte count of handed-back reads (with `counts` also the 8-byte
 * count of kept reads, and mpb_filter_poisson_device the 4-byte count of reads with a byte 255, as mpb_poisson_lambda_device
 * does).  When the count is zero nothing else crosses the link.  Otherwise the host fetches the handed-back reads' lambda / ns /
 * length -- up to 65536 reads as one block of 24-byte records the kernel wrote, more than that as the whole arrays; never a copy
 * per read --, runs the host tail on them and writes their ee / pass back before returning.
 * counts (may be NULL): n_reads, n_pass, n_fail over the final flags; n_overflow = the reads the host finished.
 *
 * mpb_poisson_finish_device: the device twin of mpb_poisson_finish_host -- lambda / ns / len on the device, results on the device.
 * d_ee may be the same array as d_lambda (each lane reads its lambda before it writes its ee).  d_ns is not written.
 */
int mpb_poisson_finish_device(mpb_ctx *ctx, const double *d_lambda, const int32_t *d_ns,
                              const int32_t *d_len, int32_t fixed_len, int64_t n,
                              const mpb_filter_params *params,
                              double *d_ee, uint8_t *d_pass, mpb_filter_counts *counts);
/* The resident Poisson filter: k_lambda + the device tail, the twin of mpb_filter_device for --error_calc poisson.  Arguments as
 * mpb_poisson_lambda_device checks them (shape, alignment, row_stride <= 2^24; a byte 255 fails the call with MPB_E_INVALID).
 * d_lambda may be NULL (lambda then lives in d_ee until the tail overwrites it); when given it receives
 * mpb_poisson_lambda_device's values. */
int mpb_filter_poisson_device(mpb_ctx *ctx, const uint8_t *d_q, int64_t n, int64_t row_stride,
                              const int32_t *d_len, int32_t fixed_len,
                              const mpb_filter_params *params,
                              double *d_ee, int32_t *d_ns, uint8_t *d_pass, double *d_lambda,
                              mpb_filter_counts *counts);

/*
 * One read, the signature-level twin of moira.py's
 *   calculate_errors_poisson(sequence, quals, alpha) -> (expected_errors, Ns)
 * ref: moira/moira.py:1637-1679.  The function's own rules, not the batch encoding's: any non-negative int is a score
 * (one outside 1..254 gets a private table entry for the call, as in mpb_calculate_errors_PB), Q0 is p = 1 (the clamp to
 * Q1 happens in process_data, moira.py:814, before the function is called), only 'N' is skipped and counted.  `ee` is
 * the raw percentile, NaN where the Python function raises OverflowError.  alpha must be in (0, 1), as the script's own
 * argument check demands (the bare function also takes 1).
 */
int mpb_calculate_errors_poisson(mpb_ctx *ctx, const char *sequence,
                                 const int32_t *quals, int32_t len,
                                 double alpha, double *ee, int32_t *ns);

/* ---- synthetic workload (BASELINE.json configs; integer-only generator) ---- */
/* Fill a device quality matrix with the counter-based synthetic model of
 * include/mpb_synth.h (identical integers on host and device).
 * fixed_len > 0: every read has fixed_len bases, d_len may be NULL.
 * fixed_len == 0: ragged, lengths drawn in [min_len, max_len] and written to d_len. */
int mpb_synth_fill_device(mpb_ctx *ctx, uint8_t *d_q, int64_t n, int64_t row_stride,
                          int32_t fixed_len, int32_t min_len, int32_t max_len,
                          int32_t *d_len, uint64_t seed, int64_t first_read);
/* The same for a named quality profile of include/mpb_synth.h: 0 = the model above (BASELINE's configs), 1 = a clean run
 * (Q33..Q40, 0.003 % ambiguous bases: the HBM-bound regime, bench.py extras.high_quality_300). */
int mpb_synth_fill_device_profile(mpb_ctx *ctx, uint8_t *d_q, int64_t n, int64_t row_stride,
                                  int32_t fixed_len, int32_t min_len, int32_t max_len,
                                  int32_t *d_len, uint64_t seed, int64_t first_read, int32_t profile);

/* ---- measurement ----------------------------------------------------------- */
/* When enabled, every launch of kernel `MPB_K_*` is bracketed by HIP events on
 * the context's stream; mpb_kernel_time() returns accumulated milliseconds and
 * the number of launches since the last reset (it synchronises the stream). */
int mpb_timing_enable(mpb_ctx *ctx, int on);
int mpb_timing_reset(mpb_ctx *ctx);
int mpb_kernel_time(mpb_ctx *ctx, int kernel_id, double *total_ms, int64_t *launches);
/* Histogram of the DP row-budget classes of the last mpb_filter_device call (or mpb_filter_host call
 * that went through the batched pipeline; the one-read-per-wave path keeps no table):
 * caps[i] = rows (J_cap) of class i, counts[i] = reads in it.  Returns the
 * number of classes written (<= max_classes).  Synchronises. */
int mpb_last_class_histogram(mpb_ctx *ctx, int32_t *caps, int64_t *counts, int32_t max_classes);
/* Row budget (J_cap) the prepass assigned to each of the first n reads of the last mpb_filter_device call
 * (0 for a read MPB_FLAG_DECISION_ONLY settled without a DP); host array of n int32.  Diagnostic: what
 * tools/class_efficiency.py uses to build single-class batches.  Synchronises. */
int mpb_last_read_budgets(mpb_ctx *ctx, int32_t *caps_out, int64_t n);
/* (Both fail with MPB_E_INVALID when the last filter call took the narrow pass: the workspace then describes the sub-batch it handed
 * back, or an earlier batch.  Ask for them after a call with MPB_FLAG_NO_NARROW.) */
/* Algorithmic DP cells of the last mpb_filter_device call made with MPB_FLAG_COUNT_CELLS (0 without it).  Synchronises. */
int mpb_last_algorithmic_cells(mpb_ctx *ctx, int64_t *cells);

/*
 * Which pass the last mpb_filter_device call took (round 5).
 * A batch of GOOD reads -- nearly every read's CDF crosses 1 - alpha within its first 2..4 rows of the table
 * (ref: moira/bernoullimodule.c:152-166,219-251: rows 0..j depend on no later row) --
 * is bound by HBM, not by FP64 issue, and the sorted pipeline would read the matrix twice.  Such a batch (>= 262144 reads,
 * default table, none of the opt-in flags) takes the NARROW PASS instead: the matrix is read once, one read per lane with
 * narrow_rows rows in registers; reads it cannot finish (more rows needed, or a lower-case 'n') are listed and run through the
 * sorted pipeline WHERE THEY LIE (round 6: its classification and sort walk the list, its DP addresses rows and results by read
 * anyway; round 5 gathered them into a dense sub-batch of their own); when they are more than half of the batch the whole batch
 * runs through the sorted pipeline instead and n_fallback reports n.  Fixed-length batches are walked in natural order.  RAGGED batches (round 6: d_len != NULL, rows of up
 * to 4096 bytes -- e.g. the contigs of the reference's paired mode, moira/moira.py:789-801) are first sorted by length inside
 * windows of 4096 consecutive reads (8 bytes per read of workspace), so that the 64 reads a wave walks together end together,
 * and only the 128-byte lines a read's bases lie in are fetched; in the sample's histogram each read then weighs its 16-byte
 * chunks, and a length outside its row is a read the pass hands back (the sorted pipeline reports it).  The choice is
 * made from a sample of at most 0.1 % of the reads (the prepass' row prediction on 256..4096 reads spread over the batch), is
 * reused while the batches of a context keep their shape and parameters (re-sampled when a pass had to hand back more reads
 * than the sample promised, and every 64 calls), and steers speed only: every read's result is the reference's bit for bit
 * whichever pass computed it.
 *   narrow_rows  0: the sorted pipeline; 2..4: the narrow pass with that many rows
 *   sampled      1 when this call drew a sample (sample_hist is then its histogram: [0] reads with a lower-case 'n', [r] reads
 *                that need r rows (r = 1..14), [15] more), 0 when it reused the previous decision
 *   n_fallback   reads the narrow pass handed to the sorted pipeline
 *   narrow_split ragged batches, narrow_rows >= 3 ("mixed rows"): how many rows a read of a given quality needs grows with its length,
 *                and the pass walks its reads sorted by length -- groups whose longest read has at most this many 16-byte chunks
 *                (safely fewer than the shortest sampled read that needed narrow_rows rows) ran with narrow_rows - 1 rows; 0: none
 *   narrow_waves the waves of the pass' persistent grid in this call (four per workgroup); 0 when the pass did not run
 * Environment MPB_NARROW_GRID_BLOCKS (a test hook, read once per call that takes the narrow pass): a value of 1 .. 2048 caps the
 * workgroups of that grid, after the library's own caps, so that a wave walks several row blocks / stream blocks / groups of a batch
 * of a few thousand reads (by itself the grid has a wave per block up to what the CUs hold at once, thousands of waves); unset or
 * any other value: no cap.
 * Every result is the same whatever the grid (only which wave walks which block changes); narrow_waves reports what was launched.
 */
typedef struct mpb_path_info {
    int32_t narrow_rows;
    int32_t sampled;
    int64_t n_fallback;
    int32_t sample_hist[16];
    int32_t narrow_split;   /* round 6, ragged batches with narrow_rows >= 3: groups of the pass whose longest read has at most this
                               many 16-byte chunks ran with narrow_rows - 1 rows (0: none) */
    int32_t narrow_waves;   /* waves of the last narrow launch (0: the pass did not run) */
} mpb_path_info;
int mpb_last_path(mpb_ctx *ctx, mpb_path_info *out);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* MOIRA_PB_H */
