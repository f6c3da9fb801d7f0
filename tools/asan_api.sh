#!/bin/bash
# CPU-only AddressSanitizer + UBSan run of the HOST-side code of the C ABI layer: packers, the Poisson tail (threaded),
# the row descriptors of the device text pack (mpb_text_rows), argument validation.  The kernels are not involved (GPU sanitizers are not available on this pool): all of it lives in
# the HIP-free unit (mpb_hostonly.cpp), which is all this builds -- no HIP header, no HIP library, no stub.
set -e
cd "$(dirname "$0")/.."
D=${TMPDIR:-/tmp}/mpb_asan; mkdir -p $D
cat > $D/main.cpp <<'CPP'
#include "moira_pb.h"
#include "mpb_hostonly.h"
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
int main()
{
    int bad = 0;
    // packers: every length from 0 to the row size, N / n / Q0, range errors
    for (int len = 0; len <= 48; len++) {
        std::vector<int32_t> q(len ? len : 1);
        std::vector<char> s(len + 1, 'A');
        s[len] = 0;
        for (int i = 0; i < len; i++) { q[i] = (i * 7) % 60; if (i % 11 == 3) s[i] = 'N'; if (i % 13 == 5) s[i] = 'n'; }
        std::vector<uint8_t> row(48, 0xAB);
        bad += mpb_pack_read(s.data(), q.data(), len, row.data(), 48) != MPB_OK;
        for (int i = 0; i < len; i++) {
            const uint8_t want = s[i] == 'N' ? 0 : s[i] == 'n' ? 255 : (q[i] ? q[i] : 1);
            bad += row[i] != want;
        }
        for (int i = len; i < 48; i++) bad += row[i] != 0;
        std::vector<char> qa(len + 1, 0);
        for (int i = 0; i < len; i++) qa[i] = (char)(33 + q[i]);
        bad += mpb_pack_read_ascii(s.data(), qa.data(), len, 33, row.data(), 48) != MPB_OK;
    }
    int32_t neg[3] = {3, -1, 4};
    uint8_t row[16];
    bad += mpb_pack_read("ACG", neg, 3, row, 16) != MPB_E_RANGE;
    int32_t big[1] = {255};
    bad += mpb_pack_read("A", big, 1, row, 16) != MPB_E_RANGE;
    bad += mpb_pack_read("ACGT", neg, 3, row, 2) != MPB_E_INVALID;
    // batch packer with truncation
    const char *seqs = "ACGTNNACGTACGTAC", *quals = "IIII##IIII!!IIII";
    int64_t off[4] = {0, 6, 6, 16};
    std::vector<uint8_t> out(3 * 16);
    int32_t lens[3];
    bad += mpb_pack_batch_ascii(seqs, quals, off, 3, 33, 8, 16, out.data(), lens) != MPB_OK;
    bad += !(lens[0] == 6 && lens[1] == 0 && lens[2] == 8);
    // the Poisson tail on a batch large enough to be split over threads, incl. lambda = 0, huge lambda (NaN), Ns, round
    const int n = 40000;
    std::vector<double> lam(n), ee(n);
    std::vector<int32_t> ns(n), len(n, 300);
    std::vector<uint8_t> ps(n);
    for (int i = 0; i < n; i++) { lam[i] = i < 10 ? 0.0 : (i % 97 == 0 ? 900.0 : 0.002 * i); ns[i] = i % 5 == 0; }
    mpb_filter_params p = {0.005, 0.01, NAN, MPB_AMBIG_TREAT_AS_ERRORS, MPB_FLAG_ROUND};
    bad += mpb_poisson_finish_host(lam.data(), ns.data(), len.data(), 0, n, &p, ee.data(), ps.data()) != MPB_OK;
    bad += !(ee[1] == 0.0 && std::isnan(ee[97]) && ps[97] == 0);
    mpb_filter_params q0 = {1.5, 0.01, NAN, 0, 0};
    bad += mpb_poisson_finish_host(lam.data(), ns.data(), nullptr, 300, n, &q0, ee.data(), ps.data()) != MPB_E_INVALID;
    bad += std::strstr(mpb_last_error(), "Alpha must be between 0 and 1") == nullptr;
    // round 4: the coded batch packer (scores above 254 get spare byte codes), incl. truncation, the full-table refusal, n = 0
    {
        const char *sq = "ACNTnGGGACGTACGT";
        int32_t ql[16] = {30, 300, 30, 0, 7, 5000, 300, 254, 253, 2147483647, 1, 2, 3, 4, 5, 6};
        int64_t off2[4] = {0, 5, 8, 16};
        std::vector<uint8_t> qo(3 * 16, 0xCD);
        int32_t ln[3], codes[256];
        bad += mpb_pack_batch_coded(sq, ql, off2, 3, 0, 16, qo.data(), ln, codes) != MPB_OK;
        bad += !(ln[0] == 5 && ln[1] == 3 && ln[2] == 8 && codes[252] == 300 && codes[251] == 5000 && codes[250] == 2147483647);
        bad += !(qo[0] == 30 && qo[1] == 252 && qo[2] == 0 && qo[3] == 1 && qo[4] == 255 && qo[5] == 0);
        bad += mpb_pack_batch_coded(nullptr, ql, off2, 3, 2, 16, qo.data(), ln, codes) != MPB_OK;
        bad += !(ln[0] == 2 && ln[1] == 2 && ln[2] == 2);
        bad += mpb_pack_batch_coded(sq, ql, off2, 0, 0, 16, qo.data(), ln, codes) != MPB_OK;
        std::vector<int32_t> full(255);
        for (int i = 0; i < 254; i++) full[i] = i + 1;
        full[254] = 300;
        int64_t off3[2] = {0, 255};
        std::vector<uint8_t> wide(256);
        bad += mpb_pack_batch_coded(nullptr, full.data(), off3, 1, 0, 256, wide.data(), ln, codes) != MPB_E_RANGE;
        int32_t negq[2] = {3, -1};
        int64_t off4[2] = {0, 2};
        bad += mpb_pack_batch_coded(nullptr, negq, off4, 1, 0, 16, qo.data(), ln, codes) != MPB_E_RANGE;
        bad += mpb_pack_batch_coded(nullptr, ql, off2, 3, 0, 8, qo.data(), ln, codes) != MPB_E_INVALID;      // stride not a multiple of 16
    }
    // the validated row descriptors of k_pack_text: a good index (sel given and NULL, truncation, sizing call), every refusal, n = 0
    {
        // four records over a text of 100 bytes; the last one's quality line ends exactly at the last byte
        int64_t ix[4][MPB_IDX_COLS] = {{0, 2, 3, 10, 16, 10}, {30, 2, 33, 7, 43, 7}, {52, 2, 55, 0, 58, 0}, {60, 2, 63, 17, 83, 17}};
        const int64_t *idx = &ix[0][0];
        mpb_text_row rows[5];
        int64_t longest = -1, badrec = 7;
        bad += mpb_text_rows(idx, 4, nullptr, 4, 100, 0, 0, nullptr, &longest, &badrec) != MPB_OK;
        bad += !(longest == 17 && badrec == -1);
        bad += mpb_text_rows(idx, 4, nullptr, 4, 100, 0, 32, rows, &longest, &badrec) != MPB_OK;
        bad += !(rows[0].seq_off == 3 && rows[0].qual_off == 16 && rows[0].len == 10 && rows[3].qual_off == 83 && rows[3].len == 17 && rows[2].len == 0);
        int64_t sel[5] = {3, 0, 0, 2, 1};
        bad += mpb_text_rows(idx, 4, sel, 5, 100, 8, 16, rows, &longest, &badrec) != MPB_OK;
        bad += !(longest == 8 && rows[0].seq_off == 63 && rows[0].len == 8 && rows[1].len == 8 && rows[2].qual_off == 16 && rows[4].len == 7);
        bad += mpb_text_rows(idx, 4, nullptr, 0, 100, 0, 16, rows, &longest, &badrec) != MPB_OK;
        bad += mpb_text_rows(nullptr, 0, nullptr, 0, 0, 0, 0, nullptr, nullptr, nullptr) != MPB_OK;
        // one byte past the text
        bad += !(mpb_text_rows(idx, 4, nullptr, 4, 99, 0, 32, rows, &longest, &badrec) == MPB_E_INVALID && badrec == 3);
        ix[1][MPB_IDX_SEQ_OFF] = 94;
        bad += !(mpb_text_rows(idx, 4, nullptr, 4, 100, 0, 32, rows, &longest, &badrec) == MPB_E_INVALID && badrec == 1);
        bad += mpb_text_rows(idx, 4, nullptr, 4, 100, 6, 32, rows, &longest, &badrec) != MPB_OK;       // ... which truncation brings back inside
        ix[1][MPB_IDX_SEQ_OFF] = -1;
        bad += !(mpb_text_rows(idx, 4, sel, 5, 100, 0, 32, rows, &longest, &badrec) == MPB_E_INVALID && badrec == 4);
        ix[1][MPB_IDX_SEQ_OFF] = 33; ix[0][MPB_IDX_QUAL_OFF] = -5;
        bad += !(mpb_text_rows(idx, 4, sel, 5, 100, 0, 32, rows, &longest, &badrec) == MPB_E_INVALID && badrec == 1);
        ix[0][MPB_IDX_QUAL_OFF] = 16;
        // sel outside the index, on either side; more rows than records without sel
        sel[2] = 4;
        bad += !(mpb_text_rows(idx, 4, sel, 5, 100, 0, 32, rows, &longest, &badrec) == MPB_E_INVALID && badrec == 2);
        sel[2] = -1;
        bad += !(mpb_text_rows(idx, 4, sel, 5, 100, 0, 32, rows, &longest, &badrec) == MPB_E_INVALID && badrec == 2);
        sel[2] = 0;
        bad += mpb_text_rows(idx, 4, nullptr, 5, 100, 0, 32, rows, &longest, &badrec) != MPB_E_INVALID;
        // a length above the row, above 65535 (a text that could hold it), and a negative one
        bad += !(mpb_text_rows(idx, 4, nullptr, 4, 100, 0, 16, rows, &longest, &badrec) == MPB_E_INVALID && badrec == 3);
        ix[2][MPB_IDX_QUAL_LEN] = 65536;
        bad += !(mpb_text_rows(idx, 4, nullptr, 4, 1 << 20, 0, 0, nullptr, &longest, &badrec) == MPB_E_INVALID && badrec == 2);
        ix[2][MPB_IDX_QUAL_LEN] = 65535;
        bad += !(mpb_text_rows(idx, 4, nullptr, 4, 1 << 20, 0, 0, nullptr, &longest, &badrec) == MPB_OK && longest == 65535);
        ix[2][MPB_IDX_QUAL_LEN] = -1;
        bad += !(mpb_text_rows(idx, 4, nullptr, 4, 100, 0, 0, nullptr, &longest, &badrec) == MPB_E_INVALID && badrec == 2);
        // offsets near INT64_MAX must not wrap
        ix[2][MPB_IDX_QUAL_LEN] = 5; ix[2][MPB_IDX_QUAL_OFF] = INT64_MAX - 2;
        bad += !(mpb_text_rows(idx, 4, nullptr, 4, 100, 0, 0, nullptr, &longest, &badrec) == MPB_E_INVALID && badrec == 2);
        bad += mpb_text_rows(idx, 4, nullptr, -1, 100, 0, 0, nullptr, &longest, &badrec) != MPB_E_INVALID;
    }
    // what the inflating entries make of a member (internal: mpb_hostonly.h).  The reason of a status word: itself up to
    // MPB_BGZF_WHY_TRAILING_BYTES, MPB_BGZF_WHY_HEADER for anything the kernel never writes (MPB_BGZF_WHY_CRC included)
    {
        for (uint32_t w = 0; w <= MPB_BGZF_WHY_TRAILING_BYTES; w++) bad += bgzf_member_reason(w) != w;
        bad += bgzf_member_reason(MPB_BGZF_WHY_CRC) != MPB_BGZF_WHY_HEADER;
        bad += bgzf_member_reason(0xffffffffu) != MPB_BGZF_WHY_HEADER;
        // three status rows: the counts add up, the longest code is a maximum (the middle row's), the status word is not counted
        const uint32_t ms[3][8] = {{0, 1, 2, 3, 100, 50, 700, 9}, {0, 0, 0, 1, 0xffffffffu, 7, 0xffffffffu, 15}, {5, 2, 0, 0, 1, 1, 3, 11}};
        mpb_bgzf_inflate_stats acc;
        memset(&acc, 0, sizeof(acc));
        for (int k = 0; k < 3; k++) bgzf_stats_add(&acc, ms[k]);
        bad += !(acc.taken == 3 && acc.members == 0 && acc.handed_back == 0 && acc.stored_blocks == 3 && acc.fixed_blocks == 2 &&
                 acc.dynamic_blocks == 4 && acc.literals == 101 + 0xffffffffll && acc.matches == 58 &&
                 acc.matched_bytes == 703 + 0xffffffffll && acc.longest_code == 15);
        // the range of the vouched-for streams: all, none (the range is left alone), mixed with the extremes in the middle, and
        // one more row widening a range that is there
        mpb_bgzf_member_row rows[5] = {{500, 0, 40, 10}, {100, 10, 30, 10}, {900, 20, 64, 0}, {300, 30, 10, 10}, {600, 40, 10, 10}};
        int64_t lo = -7, hi = -7;
        bad += !(bgzf_stream_range(rows, 5, false, &lo, &hi) && lo == 100 && hi == 964);
        for (int k = 0; k < 5; k++) rows[k].out_len = -1;
        lo = hi = -7;
        bad += !(!bgzf_stream_range(rows, 5, false, &lo, &hi) && lo == -7 && hi == -7);
        bad += bgzf_stream_range(rows, 0, false, &lo, &hi);
        rows[1].out_len = 10; rows[3].out_len = 0; rows[2].stream_off = 0; rows[0].stream_off = 5000;      // (0 and 5000: not vouched for)
        bad += !(bgzf_stream_range(rows, 5, false, &lo, &hi) && lo == 100 && hi == 310);
        rows[4].out_len = 10;
        bad += !(bgzf_stream_range(rows + 4, 1, true, &lo, &hi) && lo == 100 && hi == 610);
        bad += !(bgzf_stream_range(rows, 1, true, &lo, &hi) && lo == 100 && hi == 610);                    // (a row not vouched for widens nothing)
    }
    // env_int64: unset, empty, below the range, at its ends, above it, no number
    {
        const char *name = "MPB_ASAN_API_ENV_INT64";
        unsetenv(name);
        bad += env_int64(name, 1, 1024, 77) != 77;
        const struct { const char *text; int64_t want; } cases[] = {{"", 77}, {"0", 77}, {"-5", 77}, {"1", 1}, {"1024", 1024}, {"1025", 77},
                                                                    {"99999999999999", 77}, {"many", 77}, {"12", 12}};
        for (const auto &cs : cases) { setenv(name, cs.text, 1); bad += env_int64(name, 1, 1024, 77) != cs.want; }
        setenv(name, "268435455", 1);                        // MPB_TEXT_PIECE_BYTES' range: 0 < v < 256 MiB
        bad += env_int64(name, 1, (256ll << 20) - 1, 256ll << 20) != 268435455;
        setenv(name, "268435456", 1);
        bad += env_int64(name, 1, (256ll << 20) - 1, 256ll << 20) != 256ll << 20;
        unsetenv(name);
    }
    // the refusals the entries share: the same words with and without an entry's name in front
    {
        bad += check_fastq_offset(0) != MPB_OK || check_fastq_offset(255, "who") != MPB_OK;
        bad += check_fastq_offset(256) != MPB_E_INVALID;
        bad += std::strcmp(mpb_last_error(), "fastq_offset 256: the device pack takes offsets 0..255 (beyond them no character is a quality)") != 0;
        bad += check_fastq_offset(-1, "mpb_filter_bgzf_fastq_host") != MPB_E_INVALID;
        bad += std::strcmp(mpb_last_error(), "mpb_filter_bgzf_fastq_host: fastq_offset -1: the device pack takes offsets 0..255 (beyond them no character is a quality)") != 0;
        bad += check_text_bytes(1ll << 30) != MPB_OK || check_text_bytes((1ll << 30) + 1) != MPB_E_INVALID;
        bad += std::strcmp(mpb_last_error(), "text of 1073741825 bytes: one call takes at most 1073741824 bytes (1 GiB) of text; split the chunk") != 0;
    }
    std::printf("asan_api: %d failed checks, version %s\n", bad, mpb_version());
    return bad != 0;
}
CPP
g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -ffp-contract=off -pthread -Iinclude -Imoira_amd/csrc \
    moira_amd/csrc/mpb_hostonly.cpp $D/main.cpp -o $D/asan_api
ASAN_OPTIONS=detect_leaks=0:halt_on_error=1 UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1 $D/asan_api
