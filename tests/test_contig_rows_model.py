"""k_contig_rows' per-pair code on the host (moira_amd/csrc/mpb_contig_rows.inc through tests/helpers/contig_rows_check.cpp, built
with the address and undefined-behaviour sanitizers; nothing is preloaded): from done[] and the index of contigs that
mct_contigs_from_fastq built, the rows must be mpb_text_rows' rows for the same index, text size and stride; a pair that was
handed back is an empty read whatever its index row holds; and a damaged index row comes out with len = -1 without one load
outside the two arrays.  The kernel itself and the fused call: tests/test_gpu_contigs_filter.py."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from helpers import contig_pairs as P
from moira_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I64_MAX, I64_MIN = 2 ** 63 - 1, -2 ** 63
MAX_LENS = (0, 1, 100, 128, 129, 10000)


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("contig_rows") / "check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "moira_amd", "csrc"),
                           os.path.join(ROOT, "tests", "helpers", "contig_rows_check.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def contigs():
    """About 200 pairs of every kind and of lengths 1..384 -> (cidx, rec_cap) of the host's contigs."""
    rng = np.random.default_rng(41)
    kinds = ("overlap", "ties", "unrelated", "contained", "identical")
    lens = [(1, 1), (1, 384), (384, 1), (384, 384), (150, 150), (251, 251)] + [tuple(int(v) for v in rng.integers(1, 385, 2)) for _ in range(194)]
    pairs = [P.make_pair(rng, a, b, kinds[k % 5]) for k, (a, b) in enumerate(lens)]
    _, fidx, _, ridx, cbuf, cidx, _ = P.host_contigs(pairs)
    rec_cap = len(cbuf) // len(pairs)
    assert rec_cap == int((fidx[:, 1] + 2 * (fidx[:, 3] + ridx[:, 3])).max()) + 8
    assert np.array_equal(cidx[:, 0], np.arange(len(pairs)) * rec_cap) and (cidx[:, 3] == cidx[:, 5]).all()
    return np.ascontiguousarray(cidx, np.int64), rec_cap


def run_model(exe, tmp, idx, done, rec_cap, max_len, stride, expect_status=0):
    n = len(idx)
    fin, fout = os.path.join(str(tmp), "in.bin"), os.path.join(str(tmp), "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<3q2i", n, rec_cap, stride, max_len, 0) + np.ascontiguousarray(idx, np.int64).tobytes() +
                np.ascontiguousarray(done, np.uint8).tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert r.returncode == expect_status, r.stdout[-2000:] + r.stderr[-3000:]
    if expect_status:
        return None
    assert "%d rows, 0 loads out of bounds" % n in r.stdout
    return np.fromfile(fout, E.TEXT_ROW_DTYPE)


def stride_of(cidx, max_len):
    """The fused call's stride for these contigs (no contig is longer than its bound)."""
    longest = int(cidx[:, 5].max())
    if max_len > 0:
        longest = min(longest, max_len)
    return (max(longest, 1) + 127) // 128 * 128


@pytest.mark.parametrize("max_len", MAX_LENS)
def test_rows_are_mpb_text_rows_rows(checker, contigs, tmp_path, max_len):
    cidx, rec_cap = contigs
    n = len(cidx)
    stride = stride_of(cidx, max_len)
    want, longest = E.text_rows(cidx, None, n * rec_cap, max_len, stride)
    got = run_model(checker, tmp_path, cidx, np.ones(n, np.uint8), rec_cap, max_len, stride)
    assert got.tobytes() == want.tobytes()
    assert int(got["len"].max()) == longest == (min(int(cidx[:, 5].max()), max_len) if max_len else int(cidx[:, 5].max()))


@pytest.mark.parametrize("max_len", MAX_LENS)
def test_a_pair_that_was_handed_back_is_an_empty_read(checker, contigs, tmp_path, max_len):
    """Mixed done patterns (every third, runs, the first and the last pair): a not-done row is {0, 0, 0} -- its index row holds
    values that would be refused or would overflow, and is never read into the result -- and the done rows are mpb_text_rows'."""
    cidx, rec_cap = contigs
    n = len(cidx)
    rng = np.random.default_rng(max_len + 5)
    for pattern in (np.arange(n) % 3 != 1, rng.random(n) < 0.5, np.arange(n) >= n // 2, np.zeros(n, bool),
                    (np.arange(n) != 0) & (np.arange(n) != n - 1)):
        idx = cidx.copy()
        idx[~pattern] = rng.choice(np.array([I64_MAX, I64_MIN, -1, 0xFFFFFFFFFFFF], np.int64), (int((~pattern).sum()), 6))
        stride = stride_of(cidx, max_len)
        got = run_model(checker, tmp_path, idx, pattern.astype(np.uint8), rec_cap, max_len, stride)
        sel = np.nonzero(pattern)[0]
        want, _ = E.text_rows(idx, sel, n * rec_cap, max_len, stride) if len(sel) else (np.zeros(0, E.TEXT_ROW_DTYPE), 0)
        assert got[sel].tobytes() == want.tobytes()
        assert not got[~pattern].tobytes().strip(b"\0")


def damaged(cidx, rec_cap, max_len, stride):
    """[(what, pair, column values)]: one column (or the two lengths together) of one pair's index row damaged."""
    out = []
    for i in (0, 1, len(cidx) // 2, len(cidx) - 1):
        row = cidx[i]
        lo, hi = i * rec_cap, (i + 1) * rec_cap
        ln = min(int(row[5]), max_len) if max_len else int(row[5])
        for col in (2, 4):                                   # the sequence line, the quality line
            out += [("an offset one byte before the slot", i, {col: lo - 1}),
                    ("an end one byte past the slot", i, {col: hi - ln + 1}),
                    ("an offset in the next slot", i, {col: int(row[col]) + rec_cap}),
                    ("an offset in the previous slot", i, {col: int(row[col]) - rec_cap}),
                    ("an offset at INT64_MAX", i, {col: I64_MAX}),
                    ("an offset whose end wraps", i, {col: I64_MAX - ln + 1}),
                    ("an offset just below INT64_MAX", i, {col: I64_MAX - rec_cap}),
                    ("an offset at INT64_MIN", i, {col: I64_MIN}),
                    ("a negative offset", i, {col: -1})]
        out += [("seq_len above qual_len", i, {3: int(row[3]) + 1}),
                ("seq_len below qual_len", i, {3: int(row[3]) - 1}),
                ("qual_len alone changed", i, {5: int(row[5]) + 1}),
                ("a negative length", i, {3: -1, 5: -1}),
                ("a length at INT64_MIN", i, {3: I64_MIN, 5: I64_MIN})]
        if not max_len:                                      # (a cut length is a good length: mpb_text_rows' rule)
            out += [("a length above the stride", i, {3: stride + 1, 5: stride + 1}),
                    ("a length above 65535", i, {3: 65536, 5: 65536}),
                    ("a length at INT64_MAX", i, {3: I64_MAX, 5: I64_MAX})]
    return out


@pytest.mark.parametrize("max_len", (0, 10, 129))
def test_a_damaged_index_row_comes_out_with_length_minus_one(checker, contigs, tmp_path, max_len):
    """One kind of damage to one column per run, at four pairs (the first, the second, the middle and the last slot): each
    damaged row is {0, 0, -1}, every other row is unchanged, and no load leaves the arrays."""
    cidx, rec_cap = contigs
    n = len(cidx)
    stride = stride_of(cidx, max_len)
    clean = run_model(checker, tmp_path, cidx, np.ones(n, np.uint8), rec_cap, max_len, stride)
    cases = damaged(cidx, rec_cap, max_len, stride)
    assert len({c[0] for c in cases}) >= 14
    by_kind = {}
    for what, i, cols in cases:
        by_kind.setdefault((what, tuple(sorted(cols))), []).append((i, cols))
    for (what, _), group in by_kind.items():
        idx = cidx.copy()
        for i, cols in group:
            for c, v in cols.items():
                idx[i, c] = v
        hit = np.array(sorted({i for i, _ in group}))
        got = run_model(checker, tmp_path, idx, np.ones(n, np.uint8), rec_cap, max_len, stride)
        assert (got["len"][hit] == -1).all() and not got["seq_off"][hit].any() and not got["qual_off"][hit].any(), what
        keep = np.setdiff1d(np.arange(n), hit)
        assert got[keep].tobytes() == clean[keep].tobytes(), what
    # the widest stride a length above 65535 could hide behind
    idx = cidx.copy()
    idx[3, 3] = idx[3, 5] = 65536
    got = run_model(checker, tmp_path, idx, np.ones(n, np.uint8), 1 << 20, 0, 1 << 17)
    assert got["len"][3] == -1


def test_an_index_outside_the_arrays_fails_the_run(checker, contigs, tmp_path):
    """The accessors are the check: asked for pair n, which neither array holds, they count its loads (one of done is enough:
    it reads as not done) and the run ends with status 3 -- the status run_model asserts is 0 for every other run here."""
    cidx, rec_cap = contigs
    n = len(cidx)
    fin = os.path.join(str(tmp_path), "past.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<3q2i", n, rec_cap, 128, 0, 0) + cidx.tobytes() + np.ones(n, np.uint8).tobytes())
    r = subprocess.run([checker, fin, os.path.join(str(tmp_path), "o.bin"), "past"], capture_output=True, text=True)
    assert r.returncode == 3 and "%d rows, 1 loads out of bounds" % n in r.stdout, r.stdout + r.stderr[-2000:]


def test_the_kernel_unit_includes_the_file_the_model_runs():
    src = open(os.path.join(ROOT, "moira_amd", "csrc", "mpb_contig_kernels.hip")).read()
    inc = open(os.path.join(ROOT, "moira_amd", "csrc", "mpb_contig_rows.inc")).read()
    assert '#include "mpb_contig_rows.inc"' in src and "k_contig_rows" in src and "cr_row(out_idx, done, i, rec_cap, max_len, stride)" in src
    assert "__builtin" not in inc and "__shfl" not in inc and "threadIdx" not in inc      # no intrinsic in the per-pair file
