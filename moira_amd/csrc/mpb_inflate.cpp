// mpb_inflate.cpp -- BGZF .gz input on the device, behind the C ABI of libmoira_pb.so (include/moira_pb.h): the host entry that
// validates its arguments, builds the members' rows (mpb_bgzf_member_rows, mpb_hostonly.cpp), cuts the members into pieces, uploads
// a piece's compressed bytes and rows, launches k_bgzf_inflate (mpb_inflate_kernels.hip) on it, copies status and text back, and
// checks the CRC-32 of every taken member's text against its trailer's on a few threads.  A piece is queued on a StreamQueue
// (mpb_queue.h) and waited for once; the members' verdict is mpb_hostonly.cpp's, shared with mpb_bgzf_fastq.cpp.
// (Every mpb_* function defined here has C linkage: include/moira_pb.h declares it inside extern "C".)

#include "mpb_ctx.h"

#include <algorithm>
#include <cstring>
#include <new>
#include <thread>
#include <vector>

namespace {

const int64_t k_piece_members_max = 4096;
const int64_t k_member_bytes_max = 65536;                    // either way: BSIZE is 16 bits, ISIZE is checked

struct InflateStage {
    uint8_t *in; mpb_bgzf_member_row *rows; uint32_t *mstat; uint8_t *text;
    void layout(Carver &k, int64_t in_bytes, int64_t members, int64_t text_bytes)
    {
        k.take(in, align_up(in_bytes > 0 ? in_bytes : 1, 16));
        k.take(rows, members);
        k.take(mstat, members * MPB_INFLATE_MSTAT);
        k.take(text, align_up(text_bytes > 0 ? text_bytes : 1, 16));
    }
};

struct Piece { int64_t m0, nm, in_lo, in_hi; };             // members [m0, m0 + nm), their bytes in[in_lo, in_hi)

// fn(lo, hi) over [0, n) on a few threads (the caller's among them)
template <typename F> void on_threads(int64_t n, int64_t min_per_thread, F fn)
{
    int threads = staging_threads();
    if ((int64_t)threads > n / min_per_thread) threads = (int)(n / min_per_thread);
    if (threads <= 1) { fn((int64_t)0, n); return; }
    std::vector<std::thread> th;
    const int64_t per = (n + threads - 1) / threads;
    int64_t taken = per < n ? per : n;                       // helpers take [per, taken); the rest is done here
    try {
        th.reserve((size_t)threads);
        for (int t = 1; t < threads; t++) {
            const int64_t lo = per * t, hi = lo + per < n ? lo + per : n;
            if (lo >= n) break;
            th.emplace_back(fn, lo, hi);
            taken = hi;
        }
    } catch (...) { }                                        // no more threads to be had: this one does what is left
    fn((int64_t)0, per < n ? per : n);
    if (taken < n) fn(taken, n);
    for (auto &t : th) t.join();
}

}  // namespace

int mpb_bgzf_inflate_host(mpb_ctx *c, const uint8_t *in, int64_t in_len, const int64_t *offs, const int32_t *sizes,
                          const int64_t *out_offs, int64_t n, uint8_t *out, int64_t out_cap, uint8_t *done, uint8_t *why,
                          mpb_bgzf_inflate_stats *stats)
{
    CTXCHK(c);
    if (stats) memset(stats, 0, sizeof(*stats));
    if (n < 0 || in_len < 0 || out_cap < 0 || !out_offs || (n > 0 && (!in || !offs || !sizes || !done)))
        return fail(MPB_E_INVALID, "mpb_bgzf_inflate_host: bad arguments");
    if (n == 0) return MPB_OK;
    std::vector<mpb_bgzf_member_row> rows, prow;
    std::vector<uint32_t> crc, mstat;
    std::vector<uint8_t> reason;
    std::vector<Piece> pieces;
    const int64_t per_piece = std::min(env_int64("MPB_BGZF_INFLATE_PIECE_MEMBERS", 1, k_piece_members_max, k_piece_members_max), n);
    try {
        rows.resize((size_t)n); crc.resize((size_t)n); reason.resize((size_t)n);
        prow.resize((size_t)per_piece); mstat.resize((size_t)n * MPB_INFLATE_MSTAT);
    } catch (const std::bad_alloc &) { return fail(MPB_E_NOMEM, "out of host memory for %lld members", (long long)n); }
    int rc = mpb_bgzf_member_rows(in, in_len, offs, sizes, out_offs, n, rows.data(), crc.data(), reason.data());
    if (rc) return rc;
    if (out_offs[n] > out_cap || (out_offs[n] > 0 && !out))
        return fail(MPB_E_INVALID, "mpb_bgzf_inflate_host: out_cap %lld is below the %lld bytes of text", (long long)out_cap, (long long)out_offs[n]);
    memset(done, 0, (size_t)n);

    // pieces: consecutive members, at most per_piece of them, whose bytes of `in` and of `out` each span at most per_piece * 64 KiB
    // (members that mio_bgzf_scan found lie back to back, so only the count binds); a member that is not taken joins no range
    const int64_t span_max = per_piece * k_member_bytes_max;
    int64_t in_need = 0, text_need = 0;
    try {
        for (int64_t m0 = 0; m0 < n;) {
            Piece p{m0, 0, 0, 0};
            bool any = false;
            const int64_t out_lo = out_offs[m0];
            while (p.m0 + p.nm < n && p.nm < per_piece) {
                const int64_t k = p.m0 + p.nm;
                if (out_offs[k + 1] - out_lo > span_max && p.nm > 0) break;
                if (rows[(size_t)k].out_len >= 0) {
                    int64_t new_lo = p.in_lo, new_hi = p.in_hi;
                    bgzf_stream_range(&rows[(size_t)k], 1, any, &new_lo, &new_hi);      // (the piece's range widened by this member's)
                    if (new_hi - new_lo > span_max && p.nm > 0) break;
                    p.in_lo = new_lo; p.in_hi = new_hi; any = true;
                }
                p.nm++;
            }
            if (any && out_offs[p.m0 + p.nm] - out_lo <= span_max) {
                in_need = std::max(in_need, p.in_hi - p.in_lo);
                text_need = std::max(text_need, out_offs[p.m0 + p.nm] - out_lo);
                pieces.push_back(p);
            }
            m0 = p.m0 + p.nm;
        }
    } catch (const std::bad_alloc &) { return fail(MPB_E_NOMEM, "out of host memory for the pieces of %lld members", (long long)n); }

    mpb_bgzf_inflate_stats acc;
    memset(&acc, 0, sizeof(acc));
    if (!pieces.empty()) {
        InflateStage st{};
        if ((rc = carve(c, c->inflate_stage, [&](Carver &k) { st.layout(k, in_need, per_piece, text_need); }))) return rc;
        hipStream_t s = c->stream;
        StreamQueue q(c);                                    // (it leaves before the vectors above)
        for (const Piece &p : pieces) {
            const int64_t in_bytes = p.in_hi - p.in_lo, out_lo = out_offs[p.m0], text_bytes = out_offs[p.m0 + p.nm] - out_lo;
            for (int64_t j = 0; j < p.nm; j++) {             // the rows, relative to the piece's two ranges
                mpb_bgzf_member_row r = rows[(size_t)(p.m0 + j)];
                if (r.out_len >= 0) { r.stream_off -= p.in_lo; r.out_off -= out_lo; }
                prow[(size_t)j] = r;
            }
            q.up(st.in, in + p.in_lo, in_bytes);
            q.up(st.rows, prow.data(), p.nm * (int64_t)sizeof(mpb_bgzf_member_row));
            q.run(MPB_K_BGZF_INFLATE, [&] { mpb_launch_bgzf_inflate(st.in, in_bytes, st.rows, p.nm, st.text, text_bytes, st.mstat, s); });
            q.down(&mstat[(size_t)p.m0 * MPB_INFLATE_MSTAT], st.mstat, p.nm * MPB_INFLATE_MSTAT * (int64_t)sizeof(uint32_t));
            q.down(out + out_lo, st.text, text_bytes);
            if ((rc = q.wait("k_bgzf_inflate / hipMemcpyAsync (inflate piece)"))) return rc;
            for (int64_t j = 0; j < p.nm; j++) {
                const int64_t k = p.m0 + j;
                if (rows[(size_t)k].out_len < 0) continue;
                const uint32_t w = mstat[(size_t)k * MPB_INFLATE_MSTAT];
                reason[(size_t)k] = bgzf_member_reason(w);
                if (w == MPB_BGZF_WHY_OK) done[k] = 1;       // (until the CRC says otherwise)
            }
        }
        // the CRC-32 of every taken member's text against its trailer's
        uint8_t *reason_p = reason.data();
        const mpb_bgzf_member_row *rows_p = rows.data();
        const uint32_t *crc_p = crc.data();
        on_threads(n, 16, [=](int64_t lo, int64_t hi) {
            for (int64_t k = lo; k < hi; k++) {
                if (!done[k]) continue;
                if (bgzf_crc32(out + rows_p[k].out_off, (size_t)rows_p[k].out_len) != crc_p[k]) { done[k] = 0; reason_p[k] = MPB_BGZF_WHY_CRC; }
            }
        });
    }
    for (int64_t k = 0; k < n; k++)
        if (done[k]) bgzf_stats_add(&acc, &mstat[(size_t)k * MPB_INFLATE_MSTAT]);
    if (why) memcpy(why, reason.data(), (size_t)n);
    if (stats) { *stats = acc; stats->members = n; stats->handed_back = n - acc.taken; }
    return MPB_OK;
}
