// mpb_internal.h -- shared between the GPU-facing units of the C-ABI layer (mpb_context.cpp, mpb_resident.cpp, mpb_hostfed.cpp,
// mpb_perread.cpp, mpb_poisson.cpp) and the gfx950 kernels (mpb_kernels.hip).  Not installed; the public surface is include/moira_pb.h.
#ifndef MPB_INTERNAL_H
#define MPB_INTERNAL_H

#include <hip/hip_runtime.h>
#include "mpb_shared.h"                  // the verdict on one read, MPB_MAX_LEN, MPB_NAR_MIN_ROWS / _MAX_ROWS / _BUCKETS (HIP-free)

// ---- DP row-budget classes -------------------------------------------------------------
// A read predicted to need J rows of the DP table goes to the smallest class with
// cap >= J.  cap = G * R: G lanes cooperate on one read, each keeps R consecutive rows of the
// running probability vector in registers.  G == 1 is one read per lane.  R <= 16 everywhere so
// the whole kernel fits a small VGPR budget (many waves per SIMD hide the LUT-read latency).
// Tile classes (below) cover up to MPB_TILE_MAX_ROWS rows of the DP table: one wave, 64 lanes x 16 registers.
// A read predicted to need more rows is a WIDE read: one workgroup of up to MPB_WIDE_WAVES waves holds its running
// vector (wave w keeps rows w*1024 .. w*1024+1023), the waves run one 64-base block apart and hand the row that
// crosses a wave boundary on through an LDS stream (k_wide).  16 waves x 1024 rows = 16384 rows: what a read may NEED (about
// 16,000 expected errors); a read that needs more has no result (NaN, pass = 0).  Rounds 1-3 tied the longest read to that
// number (len + 1 <= rows, so that the fallback always covers); round 4: the kernels never cared about the length itself, a
// long read of moderate quality needs few rows, so the longest read is what the 16-bit counters of ambiguous bases hold.
#define MPB_TILE_MAX_ROWS 1024
#define MPB_WIDE_WAVES 16
#define MPB_MAX_ROWS (MPB_TILE_MAX_ROWS * MPB_WIDE_WAVES)
#define MPB_MAX_STRIDE 65536              // widest quality-matrix row (bytes)
#define MPB_SMALL_MAX_STRIDE 16384        // widest row of the one-read-per-wave kernel (a lane peels at most 256 bytes of markers)

struct MpbClass { int cap, G, R; };

// X(id, R, G): the single list the class table AND the kernel's dispatch switch are generated from
#define MPB_NCLS 32
#define MPB_CLASSES(X)                                                                       \
    X(0, 2, 1) X(1, 3, 1) X(2, 4, 1) X(3, 5, 1) X(4, 6, 1) X(5, 7, 1) X(6, 8, 1) X(7, 9, 1)  \
    X(8, 10, 1) X(9, 12, 1) X(10, 14, 1) X(11, 16, 1)                                        \
    X(12, 10, 2) X(13, 12, 2) X(14, 14, 2) X(15, 16, 2)                                      \
    X(16, 10, 4) X(17, 12, 4) X(18, 14, 4) X(19, 16, 4)                                      \
    X(20, 9, 8) X(21, 10, 8) X(22, 11, 8) X(23, 12, 8) X(24, 14, 8) X(25, 16, 8)             \
    X(26, 10, 16) X(27, 12, 16) X(28, 16, 16)                                                \
    X(29, 12, 32) X(30, 16, 32) X(31, 16, 64)

// Latency bodies of the one-read-per-wave kernel (k_small): X(id, R, G) with cap = R * G = 2^(id + 1); a read of `rows` rows takes
// id = ceil(log2(rows)) - 1.  ONE row per lane up to 64 rows (7 instructions of the wave's dependent chain per base), then 2, 4,
// 8, 16 rows per lane.  (16, 64) is a tile class as well; the others exist only here.
#define MPB_THIN_CLASSES(X)                                                                  \
    X(0, 1, 2) X(1, 1, 4) X(2, 1, 8) X(3, 1, 16) X(4, 1, 32) X(5, 1, 64) X(6, 2, 64)         \
    X(7, 4, 64) X(8, 8, 64) X(9, 16, 64)

#define MPB_CLASS_ENTRY(ID, RR, GG) {(RR) * (GG), GG, RR},
#define MPB_CLASS_TABLE { MPB_CLASSES(MPB_CLASS_ENTRY) }

// reads handled by one prepass / scatter block: MPB_PRE_ROUNDS rounds of 256 (one thread per read in
// the ranking step).  More reads per block = shorter histograms to scan.
#define MPB_PRE_ROUNDS 4
#define MPB_PRE_READS (256 * MPB_PRE_ROUNDS)
// class byte of a read the prepass already settled (MPB_FLAG_DECISION_ONLY): never scattered, never run
#define MPB_CLS_SETTLED 0x7f
// class byte of a wide read (more than MPB_TILE_MAX_ROWS rows predicted): listed for k_wide, never scattered
#define MPB_CLS_WIDE 0x7e

// Sort key of a read = (class, length bin of 2^len_shift bases): perm[] is grouped by class and, inside a class,
// by length, because a DP tile runs as long as its longest read.  Batches with one fixed length use a
// single bin.  16 bins: 64 bases wide for rows of up to 1024 bases, wider (MpbDevParams.len_shift) for longer rows.
#define MPB_LEN_SHIFT 6               // narrowest bin width: 2^6 bases
#define MPB_LEN_BINS (1024 >> MPB_LEN_SHIFT)
#define MPB_SKEYS (MPB_NCLS * MPB_LEN_BINS)

// Device-side tables produced by the scan kernel, consumed by scatter and DP kernels.
struct MpbTables {
    int32_t count[MPB_NCLS];          // reads per class
    int32_t perm_base[MPB_NCLS + 1];  // first slot of the class in perm[]
    int32_t tile_start[MPB_NCLS + 1]; // first tile of the class (tiles ordered widest class first)
    int32_t total_tiles;
    int32_t kcount[MPB_SKEYS];        // reads per sort key (class * bins + bin)
    int32_t key_base[MPB_SKEYS];      // first slot of the key in perm[]
};

// consecutive tiles one wave processes: almost always of one class, so a wave enters a class body
// (a real call that saves callee-saved VGPRs to scratch) once per chunk
#define MPB_DP_CHUNK 8

struct MpbDevParams {
    double thr;            // 1 - alpha, computed on the host in double (ref: bernoullimodule.c:244)
    double uncert;
    double maxerrors;      // NaN when unset
    float  z;              // Phi^-1(1 - alpha), prediction only
    float  zq;             // (z*z - 1) / 6,     prediction only
    float  clow;           // sqrt(2 ln(1/(1-alpha))): Chernoff lower-tail coefficient (MPB_FLAG_DECISION_ONLY)
    int32_t ambig_mode;
    uint32_t flags;
    int32_t fixed_len;     // used when d_len == nullptr
    int32_t max_len;       // upper bound of every length in the batch (<= row_stride)
    int32_t len_shift;     // length-bin width of the sort key: 2^len_shift bases, (max_len - 1) >> len_shift < MPB_LEN_BINS
};

struct MpbWorkspace {
    uint8_t  *cls;         // [n]   class id | 0x80 if the read has an upper-case N
    int32_t  *perm;        // [n + MPB_NCLS*64] read indices grouped by class
    uint16_t *perm_ns;     // [n + MPB_NCLS*64] ambiguity count of perm[k]'s read, so that the DP epilogue reads it
                           // next to the index instead of gathering ns[idx] (one line request per read)
    int32_t  *blockhist;   // [MPB_SKEYS][nblocks_pre], key-major
    MpbTables *tables;     // main pass
    MpbTables *tables2;    // overflow pass
    int32_t  *ovf_list;    // [n]
    int32_t  *ovf_count;   // [1]
    int32_t  *bad_len;     // [1] lengths in d_len outside 0..max_len seen by the prepass (sticky; the host reports and clears it)
    long long *ovf_total;  // [1] overflow re-runs summed over the chunks of one host-pipeline call
    int32_t  *wide_list;   // [n] reads the prepass classed as wide (only allocated for batches whose rows can hold > 1023 bases)
    int32_t  *wide_rows;   // [n] ... and the rows predicted for each
    int32_t  *wide_count;  // [1]
    unsigned long long *pass_count;  // [1]
    unsigned long long *alg_cells;   // [1] MPB_FLAG_COUNT_CELLS: algorithmic DP cells of the last mpb_filter_device call
    const double2 *lut;    // [256] {1-p, p'} on device
    int32_t  *nar_count;   // [1] reads the natural-order narrow pass could not finish
    int32_t  *nar_seg;     // [n + 64] ... as the waves of the pass listed them, a segment per wave
    int32_t  *nar_list;    // [n + 64] ... compacted: the dense list the sorted pipeline walks
    int32_t  *nar_wave_count;   // [MPB_NAR_MAX_WAVES] entries of each wave's segment
    int32_t  *nar_sample;  // [MPB_NAR_BUCKETS + 2] histogram of the batch sample that picks the pass (k_sample) + the chunks of the
                           // shortest sampled reads that need a third / a fourth row (ragged batches)
    // the narrow pass of RAGGED batches (k_narrow_rg, round 6; allocated by the first ragged call)
    int2     *rg_ord;      // [n + 64] {read, length} in the order the pass walks them: windows of 4096 reads sorted by length
    int32_t  *rg_gpre;     // [n / 64 + 2] cost of each group of 64 entries (from its longest read), summed up inside its window
    unsigned long long *rg_wsum, *rg_wpre;   // [n / 4096 + 2] cost of each window; exclusive prefix ([nwin] = the total)
    int32_t  *rg_gstart;   // [MPB_NAR_MAX_WAVES + 1] first group of each wave of the persistent grid (written by the pass itself)
    int32_t  *pt_count;    // [1] reads k_poisson_tail handed back to the host tail
};

// ---- natural-order narrow pass (round 5) -------------------------------------------------------
// A batch of GOOD reads (nearly every read needs <= R0 rows of the DP table, R0 = 2..4) is bound by HBM, not by FP64 issue, and
// the two-pass pipeline (classify, sort, DP in class order) then moves 2.7x the algorithmic bytes.  k_narrow<R0> instead walks
// the matrix ONCE, in natural order, one read per lane with R0 rows in registers: rows 0..R0-1 of the table are exact whatever
// the read turns out to need, so every read whose CDF crosses inside them is finished bit for bit; the others -- and every read
// with a lower-case 'n', whose table entry is a NaN in this pass -- go on a list, are gathered into a dense sub-batch and run
// through the ordinary pipeline.  The choice is made per batch from a sample of <= 0.1 % of the reads.
// Three kernels, one arithmetic (nar_run) and one end of a read (nar_finish): k_narrow_rs (a lane walks one or more rows as one
// stream of whole 128-byte lines, panels staged in registers), k_narrow (any stride: 64-byte panels through an LDS-DMA ring) and
// k_narrow_rg (ragged batches, groups of 64 reads of nearly one length).
#define MPB_NAR_MAX_WAVES 8192            // waves of the persistent k_narrow grid (256 CUs x 3 workgroups x 4 waves = 3072 on MI355X)
#define MPB_NAR_AUTO_MIN_READS (1 << 18)  // below this a batch always takes the ordinary pipeline (unless the path is forced)

#define MPB_LUT_BYTES   (256 * 16)
#define MPB_LAMBDA_MAX_STRIDE (1 << 24)     // k_lambda addresses the 64 rows of a wave with 32-bit byte offsets

// Launch wrappers (mpb_kernels.hip).  All asynchronous on `s`.
// list != nullptr (round 6): the pass (and the scatter below) runs over the n reads list[0 .. n) of the matrix, not its first n rows
void mpb_launch_prepass(const uint8_t *q, int64_t n, int64_t stride, const int32_t *len,
                        const MpbDevParams &prm, const MpbWorkspace &ws, int32_t *ns_out,
                        double *ee_out, uint8_t *pass_out, hipStream_t s, const int32_t *list = nullptr);
void mpb_launch_decode_classify(const uint8_t *seq, const uint8_t *qual, int32_t offset, uint8_t *out, int32_t *err,
                                int64_t n, int64_t stride, const int32_t *len, const MpbDevParams &prm,
                                const MpbWorkspace &ws, int32_t *ns_out, double *ee_out, uint8_t *pass_out, hipStream_t s);
void mpb_launch_encode(const uint8_t *q, int64_t n, int64_t stride, int32_t offset, uint8_t *seq, uint8_t *qual, hipStream_t s);
// k_small on inputs / outputs that live in pinned HOST memory (one runtime call per launch: no copies): the device scratch and
// the completion flags that go with it
struct MpbSmallHost {
    uint8_t *stage;        // n x stride bytes of device memory: the rows are parked here by the kernel's statistics pass
    int32_t *ns_dev;       // n ints of device memory: the ambiguity counts for the class body (the report goes to `ns`)
    uint32_t *done;        // n words of pinned host memory, or nullptr: done[i] = token once read i's results are visible
    uint32_t token;
};
void mpb_launch_small(const uint8_t *q, int64_t n, int64_t stride, const int32_t *len, const MpbDevParams &prm,
                      const MpbWorkspace &ws, int32_t *ns, double *ee, uint8_t *pass, hipStream_t s,
                      const MpbSmallHost *host = nullptr);
// The resident one-read server (k_serve; the broker's calls without a launch each): n_ent mailbox entries, one wave each.
// Everything the host and the device exchange lies in pinned HOST memory (mapped); the scratch the class body walks in HBM.
#define MPB_SERVE_STRIDE 2048            // row bytes of a mailbox entry: reads of up to 2047 bases (longer ones take the other paths)
struct alignas(64) MpbServePrm { MpbDevParams p; };      // one 64-byte line per request
struct MpbServeBox {
    // pinned (or registered) host memory: entry e of each array lies e * its byte stride behind the pointer -- dense arrays
    // (the stride is the element's size: the context's own entry, the broker's copies) or fields of the broker's
    // shared-memory slots themselves (every stride is the slot size: the workers' requests are served where they lie)
    const uint8_t *q;                    // the row (written by the host before the door word)
    int64_t stride;                      // bytes a row may hold (the length is clamped to it)
    const MpbServePrm *prm;              // the request's parameters (fixed_len / max_len are set by the wave)
    const unsigned long long *door;      // {length << 32 | token}: a token that differs from done[e] is a request
    uint32_t *done;                      // the token of the last request served
    double *ee; int32_t *ns; uint8_t *pass;      // its results (pass == 2: the row budget was missed, the host runs it alone)
    int64_t q_step, prm_step, door_step, done_step, ee_step, ns_step, pass_step;   // the byte strides of the seven
    const uint32_t *stop;                // [1] non-zero: every wave leaves
    uint32_t *exited;                    // [1] the generation of the last launch that has drained
    // device memory
    uint8_t *stage;                      // [n_ent x stride] the row, parked by the statistics pass
    int32_t *ns_dev; uint8_t *cls; int32_t *ident;   // [n_ent] what the class body reads back
    uint32_t *gone;                      // [1] waves that have left (zeroed before the launch)
    int32_t n_ent;
};
void mpb_launch_serve(const MpbServeBox &box, const double2 *lut, uint32_t generation, uint32_t lifetime_ms, hipStream_t s);
void mpb_launch_scan(int64_t n, const int32_t *len, const MpbWorkspace &ws, hipStream_t s);
void mpb_launch_scatter(int64_t n, const int32_t *len, const int32_t *ns, const MpbDevParams &prm, const MpbWorkspace &ws,
                        hipStream_t s, const int32_t *list = nullptr);
// lut_odds != nullptr (MPB_FLAG_ODDS): the main pass runs the one-FMA recurrence on that {a, r = p / (1 - p)} table (k_dp_odds)
void mpb_launch_dp(const uint8_t *q, int64_t n, int64_t stride, const int32_t *len,
                   const MpbDevParams &prm, const MpbWorkspace &ws, const int32_t *ns,
                   double *ee, uint8_t *pass, hipStream_t s, const double2 *lut_odds = nullptr);
void mpb_launch_overflow(const uint8_t *q, int64_t n, int64_t stride, const int32_t *len,
                         const MpbDevParams &prm, const MpbWorkspace &ws, const int32_t *ns,
                         double *ee, uint8_t *pass, hipStream_t s);
// wide reads of the main pass (ws.wide_list); only launched when prm.max_len + 1 > MPB_TILE_MAX_ROWS
void mpb_launch_wide(const uint8_t *q, int64_t stride, const int32_t *len, const MpbDevParams &prm,
                     const MpbWorkspace &ws, const int32_t *ns, double *ee, uint8_t *pass, hipStream_t s);
void mpb_launch_lambda(const uint8_t *q, int64_t n, int64_t stride, const int32_t *len, int32_t fixed_len,
                       const double2 *lut_ap, double *lambda, int32_t *ns, int32_t *bad, hipStream_t s);
// The device tail of --error_calc poisson (k_poisson_tail, MPB_FLAG_POISSON_DEVICE_TAIL / mpb_poisson_finish_device): lambda -> ee / pass,
// one read per lane; ee may be the array lambda lies in.  A read the kernel does not vouch for (include/moira_pb.h: lambda outside
// 0..MPB_PT_LAMBDA_MAX, a crossing in term 0 or 1 with |thr - exp(-lambda)| < MPB_PT_WINDOW, an ee next to a decision) keeps its lambda
// in ee, gets pass = 2, is counted in *handed and -- rec != nullptr -- is recorded in rec[slot] while slot < rec_cap (in no
// particular order).  *n_pass += the reads it kept.  Both counters are zeroed by the caller.
#define MPB_PT_LAMBDA_MAX 64.0            // lambda ** j <= 2^1020 for every j <= 170: the reference's OverflowError cannot occur
#define MPB_PT_WINDOW 0x1p-17             // fixed on the numpy model (tests/helpers/poisson_tail_model.py), not on the kernel
struct MpbPoissonRec { double lambda; int32_t idx, ns, len, pad_; };     // a handed-back read, as the host tail needs it
struct MpbPoissonFix { double ee; int32_t idx, pass; };                   // ... and its result on the way back
void mpb_launch_poisson_tail(const double *lambda, const int32_t *ns, const int32_t *len, int64_t n, const MpbDevParams &prm,
                             double *ee, uint8_t *pass, int32_t *handed, MpbPoissonRec *rec, int32_t rec_cap,
                             unsigned long long *n_pass, hipStream_t s);
// ee[fix[k].idx] / pass[...] = the host tail's results of m handed-back reads
void mpb_launch_poisson_patch(const MpbPoissonFix *fix, int32_t m, double *ee, uint8_t *pass, hipStream_t s);
void mpb_launch_decode(const uint8_t *seq, const uint8_t *qual, int64_t n, int64_t stride, const int32_t *len,
                       int32_t fixed_len, int32_t offset, uint8_t *out, int32_t *err, hipStream_t s);
void mpb_launch_count(const uint8_t *pass, int64_t n, const MpbWorkspace &ws, hipStream_t s);
// k_pack_text: text + validated row descriptors -> n rows of `stride` bytes, lengths, has-'N' flags (may be nullptr); status[2] (set to
// INT64_MAX by the caller) takes the smallest row position, counted from k0, with a quality below 0 / above 254.  offset in 0..255.
void mpb_launch_pack_text(const uint8_t *text, int64_t text_bytes, const mpb_text_row *rows, int64_t n, int64_t k0, int32_t offset,
                          bool lower_n_is_base, int64_t stride, uint8_t *out, int32_t *len_out, uint8_t *flags_out,
                          int64_t *status, hipStream_t s);
// the natural-order narrow pass (the context's default table), rows0 in MPB_NAR_MIN_ROWS..MPB_NAR_MAX_ROWS: fixed-length batches
// (len == nullptr: k_narrow_rs, or k_narrow for rows of no multiple of 64 bytes at three or four rows) and ragged ones (k_rag_sort,
// k_rag_scan, k_narrow_rg: rows of up to MPB_RG_MAX_STRIDE bytes; split_chunks > 0, rows0 >= 3: groups whose longest read has at
// most that many 16-byte chunks run with rows0 - 1 rows).  Finished reads get ee / ns / pass; the others end up in ws.nar_list
// (dense, in wave order; their number in ws.nar_count).  A persistent grid on n_cu CUs; rg_per_cu: the blocks per CU of the
// MPB_NRG_FORMS ragged instantiations (mpb_narrow_rg_blocks_per_cu; only read for ragged batches).
// lut_odds != nullptr (MPB_FLAG_ODDS | MPB_FLAG_ODDS_NARROW): the one-FMA twins (k_odds_nar, k_odds_nar_rs, k_odds_nar_rg) on that
// {a, r = p / (1 - p)} table; no mixed rows then (split_chunks is ignored).
// grid_cap > 0: at most that many workgroups (the test hook MPB_NARROW_GRID_BLOCKS; 0: none).  *waves: the waves of the grid.
#define MPB_RG_MAX_STRIDE 4096
#define MPB_NRG_FORMS 8                   // k_narrow_rg's MPB_NRG_EXACT_FORMS instantiations, then k_odds_nar_rg<2..4>
#define MPB_NRG_EXACT_FORMS 5
#define MPB_NAR_GRID_CAP_MAX 2048         // the largest cap the hook takes (MPB_NAR_MAX_WAVES / 4)
void mpb_launch_narrow(int rows0, int split_chunks, const uint8_t *q, int64_t n, int64_t stride, int32_t fixed_len, const int32_t *len,
                       const MpbDevParams &prm, const MpbWorkspace &ws, double *ee, int32_t *ns, uint8_t *pass, int n_cu,
                       const int *rg_per_cu, int grid_cap, int *waves, hipStream_t s, const double2 *lut_odds = nullptr);
void mpb_narrow_rg_blocks_per_cu(int per_cu[MPB_NRG_FORMS]);
// predicted row budgets of `n_sample` reads spread over the batch -> ws.nar_sample (zeroed here)
void mpb_launch_sample(const uint8_t *q, int64_t n, int64_t stride, int32_t fixed_len, const int32_t *len, const MpbDevParams &prm,
                       const MpbWorkspace &ws, int n_sample, hipStream_t s);
// k_contig (mpb_contig_kernels.hip; the arguments: mpb_contig_args.h): one wave per listed pair, lds_bytes of LDS per wave
struct MpbContigArgs;
void mpb_launch_contigs(const MpbContigArgs &a, hipStream_t s);
// k_contig_rows: done[n] and k_contig's index -> the n row descriptors of k_pack_text over the slot buffer (mpb_contig_rows.inc)
void mpb_launch_contig_rows(const int64_t *out_idx, const uint8_t *done, int64_t n, int64_t rec_cap, int32_t max_len, int64_t stride,
                            mpb_text_row *rows, hipStream_t s);
// .gz output on the device (mpb_bgzf_kernels.hip): a member's slot holds its raw-deflate stream, at most MPB_BGZF_DATA + 5 bytes
// (a stored block), written in whole 32-bit words
#define MPB_BGZF_SLOT 65536
// k_bgzf_deflate: one workgroup per member of text[text_bytes] (the allocation rounded up to 16 bytes) -> slots[m][MPB_BGZF_SLOT],
// size[m], mstat[m][4] = {block type, literals, matches, matched bytes}; tok[m][MPB_BGZF_DATA] is its token scratch
void mpb_launch_bgzf_deflate(const uint8_t *text, int64_t text_bytes, int64_t n_members, uint32_t *tok, uint8_t *slots,
                             uint32_t *size, uint32_t *mstat, hipStream_t s);
// k_bgzf_scan: off[0 .. n_members] = the exclusive prefix of size + 26 (one block)
void mpb_launch_bgzf_scan(const uint32_t *size, int64_t n_members, int64_t *off, hipStream_t s);
// k_bgzf_frame: header, stream and trailer (crc[m], ISIZE) of every member, dense, into out[out_cap]
void mpb_launch_bgzf_frame(const uint8_t *slots, const uint32_t *size, const int64_t *off, const uint32_t *crc, int64_t text_bytes,
                           int64_t n_members, int64_t out_cap, uint8_t *out, hipStream_t s);
// BGZF .gz input on the device (mpb_inflate_kernels.hip).  k_bgzf_inflate: one wave per member of rows[n_members] over in[in_bytes]
// (a 256-byte aligned block) -> its text at text + out_off (text[text_bytes]) when taken, and mstat[m][MPB_INFLATE_MSTAT] =
// {why, stored / fixed / dynamic blocks, literals, matches, matched bytes, longest code}; the rows are checked again in the kernel
#define MPB_INFLATE_MSTAT 8
void mpb_launch_bgzf_inflate(const uint8_t *in, int64_t in_bytes, const mpb_bgzf_member_row *rows, int64_t n_members, uint8_t *text,
                             int64_t text_bytes, uint32_t *mstat, hipStream_t s);
// The FASTQ record index on the device (mpb_index_kernels.hip; what a lane does: mpb_index_lane.inc).  text[text_bytes] lies in an
// allocation rounded up to 16 bytes; a tile is MPB_FQ_TILE bytes of it.
// k_fq_lines: info[n_tiles] = a tile's newlines and its flags.  k_fq_scan (one block): prefix[n_tiles] = the newlines before a tile,
// head[4] = {newlines, refusal flags (bit 0: a non-ASCII byte, bit 1: a lone carriage return), lines, 0}.  k_fq_starts:
// start[k] = the first byte of line k, for k < n_start.  k_fq_rows: records 0..n-1 from start[] -> idx[n][6], kinds[n], desc[n];
// status[4] (set to {INT64_MAX, 0, 0, 0} by the caller) = {first bad record, longest packed length of a good one, a line check failed}.
#define MPB_FQ_TILE 16384
void mpb_launch_fq_lines(const uint8_t *text, int64_t text_bytes, int64_t n_tiles, uint32_t *info, hipStream_t s);
void mpb_launch_fq_scan(const uint8_t *text, int64_t text_bytes, bool final_text, const uint32_t *info, int64_t n_tiles,
                        uint32_t *prefix, uint32_t *head, hipStream_t s);
void mpb_launch_fq_starts(const uint8_t *text, int64_t text_bytes, int64_t n_tiles, const uint32_t *prefix, const uint32_t *head,
                          uint32_t *start, int64_t n_start, hipStream_t s);
void mpb_launch_fq_rows(const uint8_t *text, int64_t text_bytes, const uint32_t *start, int64_t n_start, int64_t n, int32_t max_len,
                        int64_t *idx, uint8_t *kinds, mpb_text_row *desc, int64_t *status, hipStream_t s);
// fasta+qual input on the device (mpb_fasta_qual_kernels.hip; what a lane does: mpb_fasta_qual_lane.inc).  Record r < n is lines
// 2 r and 2 r + 1 of ftext[fbytes] and of qtext[qbytes] (allocations rounded up to 16 bytes) by fstart / qstart[n_start], k_fq_starts'
// tables, which are not trusted.  k_fa_count + k_fa_scan: size[n], prefix[n + 1], head[4] = {n_fit: the leading records whose slots
// end at or before out_cap, prefix[n_fit], prefix[n], 0}; status[4] (set to {INT64_MAX, 0, 0, 0} by the caller): [0] = the first
// record that is not taken as record << 8 | why << 1 | which.  k_fa_write: records 0..n_fit-1 into out[out_bytes], idx[.][6] and
// desc[.] (k_pack_text's descriptors over out); status[1] = the longest packed length, status[2] = 1 when a slot's place failed its
// check; nothing when status[0] is set.
void mpb_launch_fa_count(const uint8_t *ftext, int64_t fbytes, const uint32_t *fstart, const uint8_t *qtext, int64_t qbytes,
                         const uint32_t *qstart, int64_t n_start, int64_t n, int64_t out_cap, int64_t *size, int64_t *prefix,
                         int64_t *head, int64_t *status, hipStream_t s);
void mpb_launch_fa_write(const uint8_t *ftext, int64_t fbytes, const uint32_t *fstart, const uint8_t *qtext, int64_t qbytes,
                         const uint32_t *qstart, int64_t n_start, int64_t n, int32_t max_len, const int64_t *prefix, const int64_t *head,
                         uint8_t *out, int64_t out_bytes, int64_t *idx, mpb_text_row *desc, int64_t *status, hipStream_t s);
// RFC 1952's CRC-32 on the device (mpb_crc_kernels.hip; what a lane does: mpb_crc_lane.inc).  k_bgzf_crc32: one wave per range of
// ranges[n] over text[text_bytes] (a 16-byte aligned block; 0 <= len <= MPB_CRC_RANGE_MAX, any off) -> crc[k], bad[k] = 0; a range
// that does not lie inside the text is checked again in the kernel: crc[k] = 0, bad[k] = 1, nothing read
#define MPB_CRC_RANGE_MAX 65536
struct mpb_crc_range { int64_t off; int32_t len, pad; };     // 16 bytes
void mpb_launch_bgzf_crc32(const uint8_t *text, int64_t text_bytes, const mpb_crc_range *ranges, int64_t n, uint32_t *crc,
                           uint32_t *bad, hipStream_t s);
// From two device-written record indexes to k_contig's inputs (mpb_pair_kernels.hip; what a lane does: mpb_pair_lane.inc).
// k_pair_rows: rows 0..m-1 of fidx / ridx (not trusted) -> rows[m] as mpb_pair_rows writes them (a pair that fails a check: a row
// cd_row_ok refuses) and cls[m], the LDS size class by `classes` (-1: none; take == false: none at all); status[4] (set to
// {INT64_MAX, INT64_MAX, 0, 0} by the caller): [0] the first pair whose header tokens differ, [1] the first whose rows fail a check.
// k_pair_count + k_pair_scan over pairs 0..n-1: table / prefix [ceil(n / 256)][16], head[MPB_PAIR_HEAD_WORDS] = the pairs per class,
// then the classes' first places in the list; status[2] = the largest hdr_len + 2 (l1 + l2), status[3] = the largest l1 + l2 of a
// pair with a class.  k_pair_lists: list[n], every class' pairs ascending behind each other.
#define MPB_PAIR_HEAD_WORDS 32
struct MpbLdsClasses;
void mpb_launch_pair_rows(const int64_t *fidx, const int64_t *ridx, int64_t m, const uint8_t *ftext, int64_t fbytes, const uint8_t *rtext,
                          int64_t rbytes, int maxabs, bool take, const MpbLdsClasses &classes, mpb_pair_row *rows, int8_t *cls,
                          int64_t *status, hipStream_t s);
void mpb_launch_pair_count(const mpb_pair_row *rows, const int8_t *cls, int64_t n, uint32_t *table, uint32_t *prefix, uint32_t *head,
                           int64_t *status, hipStream_t s);
void mpb_launch_pair_lists(const int8_t *cls, int64_t n, const uint32_t *prefix, const uint32_t *head, int32_t *list, hipStream_t s);
// The writer's formatter on the device (mpb_format_kernels.hip; what a lane does, FmParams and the blob: mpb_format_lane.inc).
// Records sel[k] (null: k), k < nsel, of idx[p.n_records][6] over text[p.text_bytes] (an allocation rounded up to 16 bytes); the
// rows, sel, relabel_index and label_id are not trusted.  k_fmt_count + k_fmt_scan: size[nsel], prefix[nsel + 1], head[0] = the
// bytes of the formatted text; status[0] (set to INT64_MAX by the caller) = the first k whose row fails a check.  k_fmt_write:
// records k0..k1-1, clipped to bytes [win_lo, win_hi) of the formatted text, into out[win_hi - win_lo]; nothing when status[0] is set.
// ee (p.has_ee): the bits of nsel doubles, by position; aux (the report kind): three arrays read at r * p.aux_stride, by record.
struct FmParams;
void mpb_launch_fmt_count(const uint8_t *text, const int64_t *idx, const int64_t *sel, const int64_t *relabel_index,
                          const int32_t *label_id, const uint64_t *ee, const int32_t *const aux[3], int64_t nsel, const FmParams &p,
                          int64_t *size, int64_t *prefix, int64_t *head, int64_t *status, hipStream_t s);
void mpb_launch_fmt_write(const uint8_t *text, const uint8_t *blob, const int64_t *idx, const int64_t *sel,
                          const int64_t *relabel_index, const int32_t *label_id, const uint64_t *ee, const int32_t *const aux[3],
                          int64_t k0, int64_t k1, const FmParams &p,
                          const int64_t *prefix, const int64_t *status, int64_t win_lo, int64_t win_hi, uint8_t *out, hipStream_t s);
// The data-parallel part of collapse (mpb_collapse_kernels.hip; what a lane does and ClParams: mpb_collapse_lane.inc).  Records
// k < p.n_records of idx[.][6] over text[p.text_bytes] (an allocation rounded up to 16 bytes; the rows are not trusted): k_col_hash
// -> hash[n] and status[0] (set to INT64_MAX by the caller) = the first k whose row fails its check; k_col_group over table[p.cap]
// (every byte 0xFF: empty) and first[p.cap] (every byte 0xFF) -> slot[n]; k_col_rep -> rep[n].  With status[0] set, rep[k] = k.
struct ClParams;
void mpb_launch_collapse(const uint8_t *text, const int64_t *idx, const ClParams &p, uint64_t *hash, int32_t *table, uint32_t *first,
                         int64_t *slot, int32_t *rep, int64_t *status, hipStream_t s);
void mpb_launch_synth(uint8_t *q, int64_t n, int64_t stride, int32_t fixed_len, int32_t min_len,
                      int32_t max_len, int32_t *len, uint64_t seed, int64_t first_read,
                      hipStream_t s, int32_t profile = 0);

#endif
