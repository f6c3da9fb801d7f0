// mpb_ctx.h -- the context of the C ABI (struct mpb_ctx) and what the GPU-facing host units share: the error macros, the owner of
// a growable block (Buf), the carver that lays a block out (Carver), the timing span, the queue of a staged entry (StreamQueue,
// mpb_queue.h) and the few functions that cross units (mpb_context.cpp, mpb_resident.cpp, mpb_hostfed.cpp, mpb_perread.cpp,
// mpb_poisson.cpp, mpb_text.cpp, mpb_contig.cpp, mpb_index.cpp, mpb_bgzf_fastq.cpp).  Not installed.
#ifndef MPB_CTX_H
#define MPB_CTX_H

#include "../../include/moira_pb.h"
#include "mpb_internal.h"
#include "mpb_host_internal.h"
#include "mpb_hostonly.h"

#include <vector>

static_assert(sizeof(MpbPair) == sizeof(double2) && offsetof(MpbPair, y) == sizeof(double), "MpbPair is double2's layout");

static inline int hip_fail(const char *what, hipError_t e)
{
    return fail(e == hipErrorOutOfMemory ? MPB_E_NOMEM : MPB_E_HIP, "%s failed: %s", what, hipGetErrorString(e));
}
#define HIPCHK(expr)                                        \
    do {                                                    \
        hipError_t e_ = (expr);                             \
        if (e_ != hipSuccess) return hip_fail(#expr, e_);   \
    } while (0)
// ... of calls whose results were kept until a synchronisation had been made: the first that failed
#define HIPCHK_KEPT(what, e)                                \
    do {                                                    \
        if ((e) != hipSuccess) return hip_fail(what, e);    \
    } while (0)

#define CTXCHK(c)                                                     \
    do {                                                              \
        if (!(c)) return fail(MPB_E_INVALID, "%s: ctx is NULL", __func__); \
        HIPCHK(hipSetDevice((c)->device));                            \
    } while (0)

// ---- one owner for a block of device or pinned memory --------------------------------------------------------------------
// grow() is the ONLY place that frees a block to make a larger one: the runtime waits for the whole device in a free, so the
// context's stream is synchronised and the per-read entry's resident kernel is asked to leave (serve_quiesce) first.
enum BufKind { BUF_DEVICE, BUF_PINNED, BUF_MAPPED };     // hipMalloc; hipHostMalloc; hipHostMalloc, mapped into the device
struct Buf {
    BufKind kind;
    void *p = nullptr;
    int64_t cap = 0;                                     // bytes
    explicit Buf(BufKind k = BUF_DEVICE) : kind(k) {}
    Buf(const Buf &) = delete;
    Buf &operator=(const Buf &) = delete;
    ~Buf() { release(); }
    hipError_t alloc(int64_t bytes);                     // an empty block only: no wait, no free (context and server set-up)
    // at least `bytes`; a block that has to be replaced is made `alloc_bytes` large (0: bytes).  Fails with p == nullptr, cap == 0.
    int grow(mpb_ctx *c, int64_t bytes, int64_t alloc_bytes = 0);
    void release();
};

// The layout of a block: one statement list (a function of a Carver) walked twice.  Without a base it nulls the pointers and sums
// the sizes; with the block's base it hands out the pointers, each 256-byte aligned.  Size and offsets cannot disagree.
struct Carver {
    char *base;
    int64_t off = 0;
    explicit Carver(void *b = nullptr) : base((char *)b) {}
    template <typename T> void take(T *&ptr, int64_t count)
    {
        ptr = base ? (T *)(base + off) : nullptr;
        off += align_up(count * (int64_t)sizeof(T), 256);
    }
    int64_t bytes() const { return off; }
};
// block `b` laid out by `layout`, grown as needed (a block that is replaced gets `headroom` times the bytes).  When it cannot be
// had, every pointer of the layout is left null.
template <typename Layout>
static int carve(mpb_ctx *c, Buf &b, Layout &&layout, int headroom = 1)
{
    Carver size;
    layout(size);
    int rc = b.grow(c, size.bytes(), size.bytes() * headroom);
    if (rc) return rc;
    Carver place(b.p);
    layout(place);
    return MPB_OK;
}

// The small device block: the two class tables and the counters, each counter on a 64-byte line of its own (different kernels
// write them).  c->ws points at its members.
struct MpbSmallBlock {
    alignas(256) MpbTables tables;                       // main pass
    alignas(256) MpbTables tables2;                      // overflow pass
    alignas(64) int32_t ovf_count;
    alignas(64) int32_t bad_len;
    alignas(64) unsigned long long pass_count;
    alignas(64) long long ovf_total;                     // overflow re-runs summed over the chunks of one host-pipeline call
    alignas(64) int32_t wide_count;
    alignas(64) unsigned long long alg_cells;
    alignas(64) int32_t nar_count;
    alignas(64) int32_t nar_sample[MPB_NAR_BUCKETS + 2];
    alignas(64) int32_t pt_count;
};

// The pinned words the counts of a call land in (several copies, one synchronisation; nothing of it lies on a frame).
struct PinWords {
    int32_t nar_count;                                   // reads the narrow pass handed back
    int32_t n_overflow;                                  // overflow re-runs
    unsigned long long n_pass;
    int32_t bad_len;                                     // lengths outside 0..max_len
    int32_t bad255;                                      // Poisson paths: reads with a byte 255
    int32_t sample[MPB_NAR_BUCKETS + 2];                 // the sample histogram (k_sample)
    int32_t pt_handed;                                   // reads the Poisson device tail handed back
    unsigned long long pt_kept;                          // ... and the reads it kept
    long long ovf_total;                                 // host pipeline: overflow re-runs of all chunks
    int64_t text_status[2];                              // mpb_filter_text_host: k_pack_text's status, both ways
    uint32_t fq_head[4];                                 // the device index: k_fq_scan's head words {newlines, refusal flags, lines, 0}
    int64_t fq_status[4];                                // ... k_fq_rows' status, both ways; [3]: the first byte behind the last record
    uint32_t fq_head2[4];                                // mpb_contigs_filter_fastq_host: the same two blocks of the reverse text
    int64_t fq_status2[4];
    int64_t pair_status[4];                              // ... k_pair_rows' / k_pair_count's status, both ways
    uint32_t pair_head[MPB_PAIR_HEAD_WORDS];             // ... k_pair_scan's head words: the pairs per class, the classes' first places
    int64_t fmt_words[2];                                // mpb_format_text_host: k_fmt_count's status, both ways; k_fmt_scan's head word
    int64_t col_status[2];                               // mpb_collapse_text_host: k_col_hash's status, both ways
};

struct TimedSpan { int kid; hipEvent_t a, b; };

// the chunk arrays of the host-fed paths, as one block holds them: inputs (q | len), then outputs (ee | ns | pass)
struct ChunkArrays {
    uint8_t *q; int32_t *len; double *ee; int32_t *ns; uint8_t *pass;
    void in(Carver &k, int64_t m, int64_t row_stride) { k.take(q, m * row_stride); k.take(len, m); }
    void out(Carver &k, int64_t m) { k.take(ee, m); k.take(ns, m); k.take(pass, m); }
};

// One of the MPB_HOST_SLOTS chunk buffers of the host pipeline (mpb_filter_host): a device block
// (q | len | ee | ns | pass), a pinned staging block for inputs that arrive in pageable memory, a pinned
// block the outputs land in, and the three events that hand the chunk from stream to stream.
#define MPB_HOST_SLOTS 4
struct HostSlot {
    Buf dev{BUF_DEVICE}, pin_in{BUF_PINNED}, pin_out{BUF_PINNED};
    ChunkArrays d{}, hin{}, hout{};          // the chunk arrays in dev (all five), pin_in (q, len) and pin_out (ee, ns, pass)
    hipEvent_t h2d_done = nullptr, k_done = nullptr, d2h_done = nullptr;
    int64_t off = -1, m = 0;  // chunk in flight (off < 0: none)
};

struct mpb_ctx {
    int device = -1;
    hipStream_t stream = nullptr;        // kernels (and every call that is not the host pipeline)
    hipStream_t copy_stream = nullptr;   // host pipeline: H2D of the next chunk
    hipStream_t out_stream = nullptr;    // host pipeline: D2H of the previous chunk
    HostSlot slot[MPB_HOST_SLOTS];
    int copy_threads = 1;
    Buf luts{BUF_DEVICE};                // the three tables below
    double2 *d_lut = nullptr;
    double2 *d_lut_odds = nullptr;       // {1-p, p / (1-p)}: the table of MPB_FLAG_ODDS' main pass (k_dp_odds)
    double2 *d_lut_private = nullptr;    // one call's table when a read carries qualities above 254 (mpb_calculate_errors_PB)
    // workspace, grown on demand
    MpbWorkspace ws{};
    Buf ws_small{BUF_DEVICE};            // MpbSmallBlock
    Buf ws_block{BUF_DEVICE};            // the sorted pipeline's arrays
    int64_t ws_cap = 0;                  // ... sized for this many reads
    // what the last classify-at-source call produced (consumed by mpb_filter_device_classified; any other call that
    // rebuilds the workspace invalidates it)
    struct Classified {
        bool valid = false; const uint8_t *q = nullptr; int64_t n = 0, stride = 0; const int32_t *len = nullptr;
        int32_t fixed_len = 0; mpb_filter_params params{}; double *ee = nullptr; int32_t *ns = nullptr; uint8_t *pass = nullptr;
    } classified;
    Buf ws_wide{BUF_DEVICE};             // wide-read list + predicted rows, only for batches whose rows hold > 1023 bases
    int64_t ws_wide_cap = 0;
    // timing
    bool timing = false;
    std::vector<TimedSpan> spans;
    std::vector<hipEvent_t> event_pool;
    double acc_ms[MPB_K_COUNT] = {0};
    int64_t acc_n[MPB_K_COUNT] = {0};
    // the small-batch path: device staging, and pinned host scratch (inputs and outputs of one call, back to back)
    Buf stage{BUF_DEVICE};
    Buf pin_host{BUF_MAPPED};
    uint32_t small_token = 0;            // completion token of the last zero-copy k_small launch (never 0)
    // ---- natural-order narrow pass (round 5) ----
    int n_cu = 0;                        // compute units of the device (the persistent grid of k_narrow)
    bool narrow_ok = false;              // the default table satisfies a == 1 - b for every score (checked by mpb_create)
    Buf ws_nar{BUF_DEVICE};              // wave segments + dense list + per-wave counts
    int64_t ws_nar_cap = 0;
    Buf ws_rg{BUF_DEVICE}; int64_t ws_rg_cap = 0;    // the ragged pass' order entries, group costs, wave ranges (first ragged call)
    Buf pt_rec{BUF_DEVICE};              // MPB_PT_REC_CAP records of reads k_poisson_tail handed back (first device-tail call)
    int rg_per_cu[MPB_NRG_FORMS] = {0};  // blocks per CU of the ragged pass' instantiations (the first ragged call)
    Buf text_stage{BUF_DEVICE};          // mpb_filter_text_host: text | descriptors | status | one piece of the matrix | the results of the call
    Buf contig_stage{BUF_DEVICE};        // mpb_contigs_text_host: both texts | descriptors | class lists | the slots and arrays of the call
    Buf contig_tabs{BUF_DEVICE};         // ... and the two posterior tables, uploaded by the first posterior call
    bool contig_tabs_ready = false;
    Buf bgzf_stage{BUF_DEVICE};          // mpb_bgzf_compress_host: one piece of text | tokens | slots | sizes | offsets | CRCs | the framed output
    Buf inflate_stage{BUF_DEVICE};       // mpb_bgzf_inflate_host: one piece of compressed bytes | rows | status rows | the piece's text
    Buf fastq_stage{BUF_DEVICE};         // mpb_fastq_index_host / mpb_filter_fastq_host: text | tile table | prefix | head | status
    Buf fastq_index{BUF_DEVICE};         // ... and, sized from the counted lines: line starts | index rows | kinds | descriptors
                                         // (mpb_fasta_qual_index_host / mpb_filter_fasta_qual_host: both texts and the slots in the first, both line
                                         // tables, sizes, prefix, index rows and descriptors in the second)
                                         // (mpb_contigs_filter_fastq_host: both texts' shares of either block, one carve each, and the pairing block)
    Buf format_stage{BUF_DEVICE};        // mpb_format_text_host: text | index | sel | relabel_index | label_id | blob | sizes | prefix | words | one piece
    Buf format_out{BUF_DEVICE};          // ... one window of the formatted text, or the CRC ranges of one piece of its members
    Buf collapse_stage{BUF_DEVICE};      // mpb_collapse_text_host: text | index (the uploaded form's) | hash | slot | rep | status | table | first
    // the text and index the last successful mpb_filter_fastq_host / mpb_filter_bgzf_fastq_host / mpb_filter_fasta_qual_host call left in
    // the two blocks above
    // (mpb_format_text_host's resident form); gen == 0: none
    struct ResidentText {
        int64_t gen = 0, last = 0;       // the generation in force; the last one handed out
        const uint8_t *text = nullptr; int64_t text_bytes = 0; const int64_t *idx = nullptr; int64_t n = 0;
        // the contig generation (mpb_contigs_filter_fastq_host: the slots, their index and the three arrays in contig_stage)
        bool in_contig_stage = false;
        const int32_t *aux[3] = {nullptr, nullptr, nullptr};     // overlap, gaps, mismatches by record; null: the generation carries none
    } resident;
    Buf pin_mem{BUF_PINNED};
    PinWords *pin = nullptr;             // (in pin_mem)
    struct NarrowChoice {                // the last decision, reused while the batches keep their shape (it steers speed only)
        bool valid = false; int64_t n = 0, stride = 0; int32_t fixed_len = 0; double alpha = 0; uint32_t flags = 0;
        int rows0 = 0; int split = 0; int calls = 0;
        double expect_back = 0;          // share of the sample (by weight) that needs more rows than rows0 or holds an 'n'
    } nar_choice;
    mpb_path_info last_path{};
    // the class workspace (cls, tables) describes the last filtered batch as a whole: mpb_last_class_histogram, mpb_last_read_budgets
    bool classes_whole = true;
    // ---- the per-read entry's resident server (round 5; k_serve with ONE mailbox entry, see serve_one) ----
    struct CtxServe {
        bool tried = false, ok = false, running = false;
        hipStream_t stream = nullptr;
        Buf pin{BUF_MAPPED}, dev{BUF_DEVICE};
        MpbServeBox box{};
        uint32_t generation = 0, tok = 0;
        double cached_alpha = -1.0;
        MpbDevParams cached_prm;
    } serve;
};

struct Span {
    mpb_ctx *c; int kid; hipEvent_t a = nullptr, b = nullptr;
    Span(mpb_ctx *c_, int kid_) : c(c_), kid(kid_) { if (c->timing) start(); }
    void start();                        // (mpb_context.cpp, next to the event pool)
    ~Span()
    {
        if (c->timing) { (void)hipEventRecord(b, c->stream); c->spans.push_back({kid, a, b}); }
    }
};

// the calls one staged entry queues on c->stream and its one wait (written against the names above; includes no HIP header)
#include "mpb_queue.h"

// The kernels of one call run on a private copy of the table; the context's own is back in place when the call returns.
struct PrivateTable {
    mpb_ctx *c;
    bool on = false;
    explicit PrivateTable(mpb_ctx *ctx) : c(ctx) {}
    int install(const double2 *h);
    ~PrivateTable() { if (on) c->ws.lut = c->d_lut; }
};

// mpb_context.cpp
// one copy between a frame (or a vector) and the device, and the wait for it: nothing can return between the two
int copy_sync(mpb_ctx *c, void *dst, const void *src, size_t bytes, hipMemcpyKind kind);
int ensure_workspace(mpb_ctx *c, int64_t n);
int ensure_wide_workspace(mpb_ctx *c, int64_t n);
int ensure_narrow_workspace(mpb_ctx *c, int64_t n, bool ragged);
// mpb_resident.cpp
MpbDevParams make_dev_params(const mpb_filter_params *p, int32_t fixed_len, int32_t max_len);
// mpb_hostfed.cpp
void drain_pipeline(mpb_ctx *c);
int filter_host_pipeline(mpb_ctx *c, const uint8_t *q, int64_t n, int64_t row_stride, const int32_t *len, int32_t fixed_len,
                         const mpb_filter_params *params, double *ee, int32_t *ns, uint8_t *pass, mpb_filter_counts *counts,
                         int poisson);
// mpb_text.cpp: the staging block of a text call (text | descriptors | status | one piece of the matrix | the results of the call)
struct TextStage {
    uint8_t *text; mpb_text_row *rows; int64_t *status; uint8_t *q; int32_t *len; uint8_t *flags;
    double *ee; int32_t *ns; uint8_t *pass;
    void layout(Carver &k, int64_t text_bytes, int64_t n, int64_t piece_rows, int64_t stride)
    {
        k.take(text, align_up(text_bytes > 0 ? text_bytes : 1, 16));
        k.take(rows, n);
        layout_results(k, n, piece_rows, stride);
    }
    // ... of a call whose text and descriptors lie elsewhere on the device (mpb_filter_fastq_host): text and rows stay null
    void layout_results(Carver &k, int64_t n, int64_t piece_rows, int64_t stride)
    {
        k.take(status, 2);
        k.take(q, piece_rows * stride);
        k.take(len, n); k.take(flags, n);
        k.take(ee, n); k.take(ns, n); k.take(pass, n);
    }
};
// the rows of one piece of the matrix for n rows of `stride` bytes (at most 256 MiB; MPB_TEXT_PIECE_BYTES: less)
int64_t text_piece_rows(int64_t n, int64_t stride);
// The piece loop of a text call: n rows described by d_rows over d_text (both on the device; k_pack_text's contract) are packed
// into st.q and filtered piece by piece into st.len / flags / ee / ns / pass, with mpb_filter_text_host's three poisson forms and
// its order of errors (an upload the caller queued that failed; a quality out of range: MPB_E_RANGE and *bad_record, a position
// in row order; else the first filter call that failed).  It waits for the queue once per piece.
int filter_text_pieces(StreamQueue &q, const uint8_t *d_text, int64_t text_bytes, const mpb_text_row *d_rows, int64_t n, int64_t stride,
                       int64_t piece_rows, int32_t fastq_offset, int32_t lower_n_is_base, const mpb_filter_params *params,
                       int32_t poisson, const TextStage &st, int64_t *n_pass, int64_t *n_overflow, int64_t *bad_record);
// What follows the piece loop.  Where the results of n rows go on the host (len / flags may be null), and the lengths of the
// host tail when the caller wants none: declared before the queue that copies into it.
struct TextResults {
    double *ee; int32_t *ns; uint8_t *pass; int32_t *len; uint8_t *flags;
    std::vector<int32_t> len_tmp;
    int32_t *len_host() const { return len ? len : len_tmp.empty() ? nullptr : const_cast<int32_t *>(len_tmp.data()); }
};
// poisson without the device tail: the reference's scalar tail runs on the host, behind the wait
static inline bool text_host_tail(const mpb_filter_params *params, int32_t poisson)
{
    return poisson && !(params && (params->flags & MPB_FLAG_POISSON_DEVICE_TAIL));
}
// ... queued: the five copies out of st (`pass` only when the device wrote it; the lengths into len_tmp when the host tail needs
// them and r.len is null); after the wait: the host tail, and *n_pass (may be null) counted again from what it wrote
int text_results_queue(StreamQueue &q, const TextStage &st, int64_t n, bool host_tail, TextResults &r);
int text_results_tail(int64_t n, const mpb_filter_params *params, bool host_tail, const TextResults &r, int64_t *n_pass);
// ... queue, wait, tail: *n_pass is the piece loop's count going in, the call's going out
int text_results_out(StreamQueue &q, const TextStage &st, int64_t n, const mpb_filter_params *params, int32_t poisson, TextResults &r,
                     int64_t *n_pass);
// mpb_index.cpp: the device FASTQ index, shared with mpb_bgzf_fastq.cpp (which inflates the text into the index's own stage)

// text | tile table | prefix | head | status: sized from the text alone
struct FastqStage {
    uint8_t *text; uint32_t *info, *prefix, *head; int64_t *status;
    void layout(Carver &k, int64_t text_bytes, int64_t n_tiles)
    {
        k.take(text, align_up(text_bytes > 0 ? text_bytes : 1, 16));
        k.take(info, n_tiles > 0 ? n_tiles : 1);
        k.take(prefix, n_tiles > 0 ? n_tiles : 1);
        k.take(head, 4);
        k.take(status, 4);
    }
};

// line starts | index rows | kinds | descriptors: sized from the counted lines
struct FastqIndex {
    uint32_t *start; int64_t *idx; uint8_t *kinds; mpb_text_row *desc;
    void layout(Carver &k, int64_t n_start, int64_t rows)
    {
        k.take(start, n_start);
        k.take(idx, rows * MPB_IDX_COLS);
        k.take(kinds, rows);
        k.take(desc, rows);
    }
};

struct Indexed {                                             // what the device made of a text it took
    FastqStage st{};
    FastqIndex ix{};
    int64_t n = 0, rows = 0, longest = 0;                    // records; rows of the index (n, or n + 1: the offender's); longest packed length
};
// k_fq_lines, k_fq_scan and the copy of the head words to the pinned block (pin_head; null: fq_head), queued over the text that lies in
// out.st.text; after
// the caller's wait fastq_index_finish does the rest (*why != 0: handed back; it waits for what it queues); queue_index_out
// queues the copies of the index's rows, the offender's kind and the first byte behind the last record
void fastq_index_queue_head(StreamQueue &q, Indexed &out, int64_t text_bytes, int32_t final, uint32_t *pin_head = nullptr);
int fastq_index_finish(StreamQueue &q, int64_t text_bytes, int64_t max_records, int32_t max_len, int64_t idx_cap_rows, int64_t *n_needed,
                       Indexed &out, int32_t *why);
void queue_index_out(StreamQueue &q, const Indexed &in, int64_t *idx_out, uint32_t *consumed32, uint8_t *kind8);
// The filter tail of an indexed text that lies on the device (in.st.text), shared by mpb_filter_fastq_host and
// mpb_filter_bgzf_fastq_host: the two size refusals, the text call's stage, the piece loop, the index's rows and the results
// copied out behind one wait (text_out: the whole text too, or null), the out-parameters and the counts.
struct FastqFilterAsk {
    int32_t fastq_offset, lower_n_is_base; const mpb_filter_params *params; int32_t poisson;
    mpb_filter_counts *counts; int64_t *bad_record;
};
int filter_indexed(StreamQueue &q, const Indexed &in, int64_t text_bytes, uint8_t *text_out, int64_t *idx_out, int64_t *n,
                   int64_t *consumed, int32_t *bad_kind, const FastqFilterAsk &ask, TextResults &r);
// ... the text and the device-written index a successful filter_indexed left in fastq_stage / fastq_index become the context's
// resident text (a new generation); resident_drop: none.  Every entry that carves either block drops it first.
void resident_keep(mpb_ctx *c, const Indexed &in, int64_t text_bytes);
void resident_drop(mpb_ctx *c);
// ... the contig generation: the slot buffer, the device-written out_idx and the overlap / gaps / mismatches arrays a successful
// mpb_contigs_filter_fastq_host left in contig_stage.  That block belongs to the contig stage: the two entries that carve it without
// touching the index's blocks drop a generation that lies in it, and only such a one (resident_drop_contigs).
void resident_keep_contigs(mpb_ctx *c, const uint8_t *slots, int64_t text_bytes, const int64_t *idx, int64_t n, const int32_t *overlap,
                           const int32_t *gaps, const int32_t *mism);
void resident_drop_contigs(mpb_ctx *c);
// mpb_bgzf.cpp: one piece of text | tokens | slots | sizes | status rows | CRCs | offsets | the framed output, and what the host
// keeps of a piece; shared with mpb_format.cpp, whose pieces of text are written where the kernels read them
struct BgzfStage {
    uint8_t *text; uint32_t *tok; uint8_t *slots; uint32_t *size, *mstat, *crc; int64_t *off; uint8_t *out;
    void layout(Carver &k, int64_t members)
    {
        k.take(text, align_up(members * (int64_t)MPB_BGZF_DATA, 16));
        k.take(tok, members * (int64_t)MPB_BGZF_DATA);
        k.take(slots, members * (int64_t)MPB_BGZF_SLOT);
        k.take(size, members); k.take(mstat, members * 4); k.take(crc, members);
        k.take(off, members + 1);
        k.take(out, members * ((int64_t)MPB_BGZF_DATA + 31));
    }
};
struct BgzfHost {
    std::vector<uint32_t> crc, mstat;                        // crc: the members' CRCs, then the device's refusal marks
    std::vector<int64_t> off;
    int reserve(int64_t per_piece);
};
// the members of one piece (MPB_BGZF_PIECE_MEMBERS; at most 1024)
int64_t bgzf_piece_members(int64_t members);
int bgzf_compress_piece(StreamQueue &q, const BgzfStage &st, int64_t tb, int64_t nm, const uint8_t *host_text,
                        const mpb_crc_range *d_ranges, uint32_t *d_bad, BgzfHost &h, uint8_t *out, int64_t out_room, int64_t *got_out,
                        mpb_bgzf_stats *stats);
// mpb_perread.cpp: the per-read entry's resident kernel leaves (before anything is freed: the runtime waits for the whole
// device there); ... and its stream and blocks go
void serve_quiesce(mpb_ctx *c);
void serve_free(mpb_ctx *c);

#endif
