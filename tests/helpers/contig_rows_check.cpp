// Host twin of k_contig_rows (moira_amd/csrc/mpb_contig_kernels.hip): the per-pair code of moira_amd/csrc/mpb_contig_rows.inc
// compiled for the host and run once per pair, as the kernel's threads run it.  The two arrays it reads -- done[n] and the
// index int64[n][6] -- lie in heap blocks of exactly their size and are read through accessors that check the element's
// position: a position outside either array fails the run (exit status 3), and tests/test_contig_rows_model.py builds this
// program with the address and undefined-behaviour sanitizers, so an overflow in the offset arithmetic fails it too.
//
// Input (argv[1]): little-endian  int64 n, rec_cap, stride;  int32 max_len, pad;  int64 idx[n][6];  uint8 done[n].
// Output (argv[2]): mpb_text_row rows[n] (24 bytes each).  Prints "<n> rows, 0 loads out of bounds".
// argv[3] == "past" (the test of the accessors themselves): pair n, which neither array holds, is asked for as well; the
// accessors count its loads without making them, and the run fails.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "moira_pb.h"

static int64_t g_n = 0;
static long g_oob = 0;
#define CR_FN static inline
static inline int cr_done(const uint8_t *done, int64_t i)
{
    if (i < 0 || i >= g_n) { g_oob++; return 0; }
    return done[i];
}
static inline int64_t cr_idx(const int64_t *out_idx, int64_t k)
{
    if (k < 0 || k >= g_n * MPB_IDX_COLS) { g_oob++; return 0; }
    return out_idx[k];
}
#include "mpb_contig_rows.inc"

int main(int argc, char **argv)
{
    if (argc != 3 && argc != 4) { fprintf(stderr, "usage: %s cases.bin rows.bin\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int64_t head[3];
    int32_t tail[2];
    if (fread(head, 8, 3, f) != 3 || fread(tail, 4, 2, f) != 2) { fprintf(stderr, "short header\n"); return 2; }
    const int64_t n = head[0], rec_cap = head[1], stride = head[2];
    const int32_t max_len = tail[0];
    if (n < 0 || n > (1 << 24) || rec_cap <= 0) { fprintf(stderr, "bad header\n"); return 2; }
    g_n = n;
    // (new[] of the exact sizes: the sanitizer sees one element past either array)
    int64_t *idx = new int64_t[(size_t)n * MPB_IDX_COLS + 0];
    uint8_t *done = new uint8_t[(size_t)n + 0];
    if (fread(idx, 8, (size_t)n * MPB_IDX_COLS, f) != (size_t)n * MPB_IDX_COLS || fread(done, 1, (size_t)n, f) != (size_t)n) {
        fprintf(stderr, "short input\n");
        return 2;
    }
    fclose(f);
    std::vector<mpb_text_row> rows((size_t)n);
    for (int64_t i = 0; i < n; i++) rows[(size_t)i] = cr_row(idx, done, i, rec_cap, max_len, stride);
    if (argc == 4 && argv[3][0] == 'p') (void)cr_row(idx, done, n, rec_cap, max_len, stride);
    delete[] idx;
    delete[] done;
    FILE *o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 2; }
    if (n && fwrite(rows.data(), sizeof(mpb_text_row), (size_t)n, o) != (size_t)n) { fprintf(stderr, "short write\n"); return 2; }
    fclose(o);
    printf("%lld rows, %ld loads out of bounds\n", (long long)n, g_oob);
    return g_oob ? 3 : 0;
}
