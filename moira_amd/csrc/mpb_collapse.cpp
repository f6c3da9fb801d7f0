// mpb_collapse.cpp -- the data-parallel part of the collapse of identical sequences on the device, behind the C ABI of
// libmoira_pb.so (include/moira_pb.h): mpb_collapse_text_host takes a text and its record index, uploaded or what the last
// filter call left on the device (the resident form, in mpb_format_text_host's words), and hands back every record's
// CPython-2.7 string hash and the first record of the chunk with the same sequence.  mio_collapse_add_grouped (csrc/fastio.cpp)
// takes both.  The kernels are mpb_collapse_kernels.hip (k_col_hash, k_col_group, k_col_rep, inside MPB_K_PACK_TEXT's span: they
// have no id of their own); what a lane does, and the row check the host makes first, are mpb_collapse_lane.inc.  The entry
// queues on one StreamQueue (mpb_queue.h).
// (Every mpb_* function defined here has C linkage: include/moira_pb.h declares it inside extern "C".)

#include "mpb_ctx.h"

#include <cstring>

// the lane code on the host: cl_row is the validation of an uploaded index (nothing else of it is called here)
#define CL_FN static inline
#define CL_LD_I64(p, k) ((p)[k])
#define CL_LD_U64(p, k) ((p)[k])
#define CL_LD_U32(p, k) ((p)[k])
#define CL_LD_SLOT(p, k) ((p)[k])
#define CL_LD16(text, off) cl_hload16((text) + (off))
#define CL_ST_U64(p, k, v) ((p)[k] = (v))
#define CL_ST_I32(p, k, v) ((p)[k] = (v))
#define CL_ST_SLOT(p, k, v) ((p)[k] = (v))
#define CL_CAS_I32(p, s, want, v) cl_hcas((p) + (s), (want), (v))
#define CL_MIN_U32(p, s, v) ((void)((p)[s] = (p)[s] < (v) ? (p)[s] : (v)))
struct cl_w16;
static inline cl_w16 cl_hload16(const uint8_t *p);
static inline int32_t cl_hcas(int32_t *p, int32_t want, int32_t v)
{
    const int32_t seen = *p;
    if (seen == want) *p = v;
    return seen;
}
#include "mpb_collapse_lane.inc"
static inline cl_w16 cl_hload16(const uint8_t *p)
{
    cl_w16 o;
    memcpy(o.w, p, 16);
    return o;
}

namespace {

// text | index (the uploaded form's two) | hash | slot | rep | status | table | first
struct CollapseStage {
    uint8_t *text; int64_t *idx; uint64_t *hash; int64_t *slot; int32_t *rep; int64_t *status; int32_t *table; uint32_t *first;
    void layout(Carver &k, int64_t text_bytes, int64_t n, int64_t cap, bool uploaded)
    {
        if (uploaded) {
            k.take(text, align_up(text_bytes > 0 ? text_bytes : 1, 16));
            k.take(idx, n * MPB_IDX_COLS);
        }
        k.take(hash, n);
        k.take(slot, n);
        k.take(rep, n);
        k.take(status, 2);
        k.take(table, cap);                                  // (the two lie behind each other: one memset sets both)
        k.take(first, cap);
    }
};

}  // namespace

int mpb_collapse_text_host(mpb_ctx *c, const char *text, int64_t text_bytes, const int64_t *idx, int64_t n_records, int64_t resident,
                           int32_t max_len, uint64_t *hash, int32_t *rep, int64_t *bad_record)
{
    // 1. the arguments: what is wrong with them is said with or without a device
    if (bad_record) *bad_record = -1;
    const bool uploaded = resident == 0;
    if (!bad_record || n_records < 0 || text_bytes < 0 || (n_records > 0 && (!hash || !rep)))
        return fail(MPB_E_INVALID, "mpb_collapse_text_host: bad arguments (a NULL where a pointer is needed, or a negative size)");
    if (resident < 0) return fail(MPB_E_INVALID, "mpb_collapse_text_host: resident %lld is no generation", (long long)resident);
    if (uploaded ? (!idx || (text_bytes > 0 && !text)) : (text != nullptr || idx != nullptr))
        return fail(MPB_E_INVALID, "mpb_collapse_text_host: either text and idx (resident == 0) or the resident text's generation, not both or neither");
    if (max_len < 0) return fail(MPB_E_INVALID, "mpb_collapse_text_host: max_len %d is negative", (int)max_len);
    if (n_records > 0x7fffffffll)
        return fail(MPB_E_INVALID, "mpb_collapse_text_host: %lld records: at most 2147483647 (rep is an int32)", (long long)n_records);
    int rc;
    if (uploaded && (rc = check_text_bytes(text_bytes))) return rc;
    ClParams p;
    memset(&p, 0, sizeof(p));
    p.n_records = n_records; p.text_bytes = text_bytes; p.max_len = max_len;
    // 2. the rows of an uploaded index, before anything goes up: the kernel's own check, made here first
    if (uploaded)
        for (int64_t k = 0; k < n_records; k++) {
            ClRow r;
            if (!cl_row(idx, k, p, &r)) {
                *bad_record = k;
                return fail(MPB_E_INVALID, "mpb_collapse_text_host: record %lld fails a check (the sequence's offset and length against the text)",
                            (long long)k);
            }
        }
    CTXCHK(c);
    if (!uploaded) {
        if (resident != c->resident.gen)
            return fail(MPB_E_INVALID, "mpb_collapse_text_host: text %lld is not resident (the context holds %lld; 0: none)",
                        (long long)resident, (long long)c->resident.gen);
        if (n_records != c->resident.n)
            return fail(MPB_E_INVALID, "mpb_collapse_text_host: n_records %lld is not the resident index's %lld", (long long)n_records,
                        (long long)c->resident.n);
        p.text_bytes = c->resident.text_bytes;
    }
    if (n_records == 0) return MPB_OK;
    // 3. the owner slots: a power of two, at least 2 n (and 16)
    p.cap_shift = 60;
    while (((int64_t)1 << (64 - p.cap_shift)) < 2 * n_records) p.cap_shift--;
    p.cap = (int64_t)1 << (64 - p.cap_shift);
    CollapseStage st{};
    if ((rc = carve(c, c->collapse_stage, [&](Carver &k) { st.layout(k, text_bytes, n_records, p.cap, uploaded); }))) return rc;
    const uint8_t *d_text = uploaded ? st.text : c->resident.text;
    const int64_t *d_idx = uploaded ? st.idx : c->resident.idx;
    int64_t *status = c->pin->col_status;
    StreamQueue q(c);
    if (uploaded) {
        q.up(st.text, text, text_bytes);
        q.up(st.idx, idx, n_records * MPB_IDX_COLS * (int64_t)sizeof(int64_t));
    }
    status[0] = INT64_MAX; status[1] = 0;
    q.up(st.status, status, 2 * sizeof(int64_t));
    q.ones(st.table, (int64_t)((uint8_t *)(st.first + p.cap) - (uint8_t *)st.table));
    q.run(MPB_K_PACK_TEXT, [&] { mpb_launch_collapse(d_text, d_idx, p, st.hash, st.table, st.first, st.slot, st.rep, st.status, c->stream); });
    q.down(status, st.status, 2 * sizeof(int64_t));
    q.down(hash, st.hash, n_records * (int64_t)sizeof(uint64_t));
    q.down(rep, st.rep, n_records * (int64_t)sizeof(int32_t));
    if ((rc = q.wait("hipMemcpyAsync (collapse uploads) / k_col_hash / k_col_group / k_col_rep"))) return rc;
    if (status[0] != INT64_MAX) {
        *bad_record = status[0];
        return fail(MPB_E_INVALID, "mpb_collapse_text_host: the kernel refused record %lld%s", (long long)status[0],
                    uploaded ? "" : " of the resident index (never expected)");
    }
    return MPB_OK;
}
