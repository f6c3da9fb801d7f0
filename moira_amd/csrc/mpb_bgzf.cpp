// mpb_bgzf.cpp -- .gz output on the device, behind the C ABI of libmoira_pb.so (include/moira_pb.h): the host entry that validates
// its arguments, cuts the text into pieces of whole BGZF members, uploads a piece, launches k_bgzf_deflate, k_bgzf_scan and
// k_bgzf_frame (mpb_bgzf_kernels.hip) on it, computes the members' CRC-32 on the host while the first two run, and copies the
// dense framed stream back.  A piece is queued on a StreamQueue (mpb_queue.h) and waited for twice: once for the sizes, once
// for the stream.  mpb_bgzf_bound is host-only (mpb_hostonly.cpp).
// (Every mpb_* function defined here has C linkage: include/moira_pb.h declares it inside extern "C".)

#include "mpb_ctx.h"

#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

namespace {

const int64_t k_piece_members_max = 1024;

}  // namespace

int64_t bgzf_piece_members(int64_t members)
{
    return std::min(env_int64("MPB_BGZF_PIECE_MEMBERS", 1, k_piece_members_max, k_piece_members_max), members);
}

int BgzfHost::reserve(int64_t per_piece)
{
    try { crc.resize((size_t)per_piece * 2); mstat.resize((size_t)per_piece * 4); off.resize((size_t)per_piece + 1); }
    catch (const std::bad_alloc &) { return fail(MPB_E_NOMEM, "out of host memory for %lld members", (long long)per_piece); }
    return MPB_OK;
}

// One piece: the nm members of the tb bytes of text that lie in st.text, framed into out[out_room]; *got: their bytes.  The
// members' CRC-32 comes from the host's copy of the text while the first two kernels run (host_text), or -- the text was made on
// the device -- from k_bgzf_crc32 over d_ranges (inside MPB_K_BGZF_DEFLATE's span: the kernel has no id of its own).
int bgzf_compress_piece(StreamQueue &q, const BgzfStage &st, int64_t tb, int64_t nm, const uint8_t *host_text,
                        const mpb_crc_range *d_ranges, uint32_t *d_bad, BgzfHost &h, uint8_t *out, int64_t out_room, int64_t *got_out,
                        mpb_bgzf_stats *stats)
{
    hipStream_t s = q.c->stream;
    int rc;
    const int64_t piece_cap = tb + 31 * nm;
    q.run(MPB_K_BGZF_DEFLATE, [&] {
        mpb_launch_bgzf_deflate(st.text, tb, nm, st.tok, st.slots, st.size, st.mstat, s);
        if (!host_text) mpb_launch_bgzf_crc32(st.text, tb, d_ranges, nm, st.crc, d_bad, s); });
    q.run(MPB_K_BGZF_SCAN, [&] { mpb_launch_bgzf_scan(st.size, nm, st.off, s); });
    if (host_text) {
        if (q.ok()) bgzf_member_crcs(host_text, tb, nm, h.crc.data());      // while the kernels run
        q.up(st.crc, h.crc.data(), nm * (int64_t)sizeof(uint32_t));
    } else {
        q.down(h.crc.data() + nm, d_bad, nm * (int64_t)sizeof(uint32_t));
    }
    q.run(MPB_K_BGZF_FRAME, [&] { mpb_launch_bgzf_frame(st.slots, st.size, st.off, st.crc, tb, nm, piece_cap, st.out, s); });
    q.down(h.off.data(), st.off, (nm + 1) * (int64_t)sizeof(int64_t));
    q.down(h.mstat.data(), st.mstat, nm * 4 * (int64_t)sizeof(uint32_t));
    if ((rc = q.wait("k_bgzf_deflate / k_bgzf_frame / hipMemcpyAsync (bgzf piece)"))) return rc;
    if (!host_text)
        for (int64_t m = 0; m < nm; m++)
            if (h.crc[(size_t)(nm + m)] != 0) return fail(MPB_E_HIP, "k_bgzf_crc32 refused member %lld of a piece (never expected)", (long long)m);
    const int64_t got = h.off[(size_t)nm];
    if (got < 26 * nm || got > piece_cap || got > out_room)
        return fail(MPB_E_HIP, "bgzf_compress_piece: a piece of %lld members came back with %lld bytes (bound %lld)",
                    (long long)nm, (long long)got, (long long)piece_cap);
    q.down(out, st.out, got);
    if ((rc = q.wait("hipMemcpyAsync (bgzf output)"))) return rc;
    *got_out = got;
    if (stats) {
        for (int64_t m = 0; m < nm; m++) {
            const uint32_t *ms = &h.mstat[(size_t)m * 4];
            stats->members++;
            if (ms[0] == 2) stats->dynamic++; else if (ms[0] == 1) stats->fixed++; else stats->stored++;
            stats->literals += ms[1]; stats->matches += ms[2]; stats->matched_bytes += ms[3];
        }
    }
    return MPB_OK;
}

int mpb_bgzf_compress_host(mpb_ctx *c, const char *text, int64_t text_bytes, uint8_t *out, int64_t out_cap, int64_t *out_bytes,
                           mpb_bgzf_stats *stats)
{
    CTXCHK(c);
    if (out_bytes) *out_bytes = 0;
    if (stats) memset(stats, 0, sizeof(*stats));
    if (text_bytes < 0 || out_cap < 0 || !out_bytes || (text_bytes > 0 && (!text || !out)))
        return fail(MPB_E_INVALID, "mpb_bgzf_compress_host: bad arguments");
    int64_t bound = 0;
    int rc = mpb_bgzf_bound(text_bytes, &bound);
    if (rc) return rc;
    if (out_cap < bound)
        return fail(MPB_E_INVALID, "mpb_bgzf_compress_host: out_cap %lld is below mpb_bgzf_bound's %lld", (long long)out_cap, (long long)bound);
    if (text_bytes == 0) return MPB_OK;
    const int64_t members = (text_bytes + MPB_BGZF_DATA - 1) / MPB_BGZF_DATA;
    const int64_t per_piece = bgzf_piece_members(members);
    BgzfHost h;
    if ((rc = h.reserve(per_piece))) return rc;
    BgzfStage st{};
    if ((rc = carve(c, c->bgzf_stage, [&](Carver &k) { st.layout(k, per_piece); }))) return rc;
    int64_t written = 0;
    StreamQueue q(c);                                        // (it leaves before the vectors above)
    for (int64_t m0 = 0; m0 < members; m0 += per_piece) {
        const int64_t nm = std::min(per_piece, members - m0);
        const int64_t t0 = m0 * (int64_t)MPB_BGZF_DATA;
        const int64_t tb = std::min(text_bytes - t0, nm * (int64_t)MPB_BGZF_DATA);
        int64_t got = 0;
        q.up(st.text, text + t0, tb);                        // the upload; the rest is the piece's, wherever its text came from
        if ((rc = bgzf_compress_piece(q, st, tb, nm, (const uint8_t *)text + t0, nullptr, nullptr, h, out + written, out_cap - written,
                                      &got, stats))) return rc;
        written += got;
    }
    *out_bytes = written;
    return MPB_OK;
}
