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

}  // namespace

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
    const int64_t per_piece = std::min(env_int64("MPB_BGZF_PIECE_MEMBERS", 1, k_piece_members_max, k_piece_members_max), members);
    std::vector<uint32_t> crc, mstat;
    std::vector<int64_t> off;
    try { crc.resize((size_t)per_piece); mstat.resize((size_t)per_piece * 4); off.resize((size_t)per_piece + 1); }
    catch (const std::bad_alloc &) { return fail(MPB_E_NOMEM, "out of host memory for %lld members", (long long)per_piece); }
    BgzfStage st{};
    if ((rc = carve(c, c->bgzf_stage, [&](Carver &k) { st.layout(k, per_piece); }))) return rc;
    hipStream_t s = c->stream;
    int64_t written = 0;
    StreamQueue q(c);                                        // (it leaves before the vectors above)
    for (int64_t m0 = 0; m0 < members; m0 += per_piece) {
        const int64_t nm = std::min(per_piece, members - m0);
        const int64_t t0 = m0 * (int64_t)MPB_BGZF_DATA;
        const int64_t tb = std::min(text_bytes - t0, nm * (int64_t)MPB_BGZF_DATA);
        const int64_t piece_cap = tb + 31 * nm;
        q.up(st.text, text + t0, tb);
        q.run(MPB_K_BGZF_DEFLATE, [&] { mpb_launch_bgzf_deflate(st.text, tb, nm, st.tok, st.slots, st.size, st.mstat, s); });
        q.run(MPB_K_BGZF_SCAN, [&] { mpb_launch_bgzf_scan(st.size, nm, st.off, s); });
        if (q.ok()) bgzf_member_crcs((const uint8_t *)text + t0, tb, nm, crc.data());      // while the kernels run
        q.up(st.crc, crc.data(), nm * (int64_t)sizeof(uint32_t));
        q.run(MPB_K_BGZF_FRAME, [&] { mpb_launch_bgzf_frame(st.slots, st.size, st.off, st.crc, tb, nm, piece_cap, st.out, s); });
        q.down(off.data(), st.off, (nm + 1) * (int64_t)sizeof(int64_t));
        q.down(mstat.data(), st.mstat, nm * 4 * (int64_t)sizeof(uint32_t));
        if ((rc = q.wait("k_bgzf_deflate / k_bgzf_frame / hipMemcpyAsync (bgzf piece)"))) return rc;
        const int64_t got = off[(size_t)nm];
        if (got < 26 * nm || got > piece_cap || written + got > out_cap)
            return fail(MPB_E_HIP, "mpb_bgzf_compress_host: a piece of %lld members came back with %lld bytes (bound %lld)",
                        (long long)nm, (long long)got, (long long)piece_cap);
        q.down(out + written, st.out, got);
        if ((rc = q.wait("hipMemcpyAsync (bgzf output)"))) return rc;
        written += got;
        if (stats) {
            for (int64_t m = 0; m < nm; m++) {
                const uint32_t *ms = &mstat[(size_t)m * 4];
                stats->members++;
                if (ms[0] == 2) stats->dynamic++; else if (ms[0] == 1) stats->fixed++; else stats->stored++;
                stats->literals += ms[1]; stats->matches += ms[2]; stats->matched_bytes += ms[3];
            }
        }
    }
    *out_bytes = written;
    return MPB_OK;
}
