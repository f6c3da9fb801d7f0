"""The device CRC-32's lane code on the host (moira_amd/csrc/mpb_crc_lane.inc through tests/helpers/crc_lane_check.cpp, built with
-fsanitize=address,undefined together with csrc/mpb_hostonly.cpp and run as a program; nothing is preloaded): the ranges of
tests/helpers/crc_ranges.py go through k_bgzf_crc32's steps with the 64 lane states of a wave in lockstep and loads checked
against the lane's slice.  The program compares every range with bgzf_crc32 and with the zlib.crc32 value passed in; two
sensitivity builds must fail that comparison.  The kernel itself: tests/test_gpu_crc32.py."""
import os
import shutil
import struct
import subprocess
import zlib

import pytest

from helpers import crc_ranges as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLEAN = " 0 loads out of bounds, 0 differ from bgzf_crc32, 0 differ from zlib.crc32, 0 table or factor words differ"


def build(tmp, *defines):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = os.path.join(str(tmp), "check")
    csrc = os.path.join(ROOT, "moira_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "include"), "-I", csrc] + list(defines) +
                          [os.path.join(ROOT, "tests", "helpers", "crc_lane_check.cpp"), os.path.join(csrc, "mpb_hostonly.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return build(tmp_path_factory.mktemp("crc_model"))


def run(exe, tmp, cases):
    """cases: [(name, text, [(off, len)])] -> (exit status, stdout, [[(crc, bad)] per case])."""
    blob = [struct.pack("<i", len(cases))]
    for _, text, ranges in cases:
        blob += [struct.pack("<q2i", len(text), len(ranges), 0), text]
        for off, ln in ranges:
            inside = 0 <= off and 0 <= ln and off + ln <= len(text)
            blob.append(struct.pack("<qiI", off, ln, zlib.crc32(text[off:off + ln]) if inside else 0))
    fin, fout = os.path.join(str(tmp), "cases.bin"), os.path.join(str(tmp), "out.bin")
    with open(fin, "wb") as f:
        f.write(b"".join(blob))
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    raw = open(fout, "rb").read()
    got, at = [], 0
    for _, _, ranges in cases:
        got.append([struct.unpack_from("<2I", raw, at + 8 * k) for k in range(len(ranges))])
        at += 8 * len(ranges)
    return r.returncode, r.stdout + r.stderr[-3000:], got


def check(exe, tmp, cases):
    rc, out, got = run(exe, tmp, cases)
    assert rc == 0 and CLEAN in out, out
    for (name, text, ranges), g in zip(cases, got):
        assert [c for c, _ in g] == [zlib.crc32(text[o:o + n]) for o, n in ranges], name
        assert not any(bad for _, bad in g), name
    return got


def all_cases():
    return [R.placed(0), R.placed(1)] + R.constant_texts() + R.flipped() + [R.overlapping(300)]


def test_the_helper_lists_are_what_they_claim():
    name, text, ranges = R.placed(0)
    assert len(text) % 16 == 15 and max(o + n for o, n in ranges) == len(text)
    for n in (0, 1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 31, 32, 33, 1023, 1024, 1025, 2047, 2049, 65535, 65536):
        assert {(o, n) for o in range(16)} <= set(ranges) and (len(text) - n, n) in ranges
    zeros = R.constant_texts()[0]
    assert len({zlib.crc32(zeros[1][:n]) for n in range(9)}) == 9
    assert len(R.flipped()) == 1 + 2 * 64


def test_placed_ranges_equal_zlib(checker, tmp_path):
    check(checker, tmp_path, [R.placed(0), R.placed(1)])


def test_constant_texts_and_overlapping_ranges(checker, tmp_path):
    got = check(checker, tmp_path, R.constant_texts() + [R.overlapping(300)])
    assert len({c for c, _ in got[0][:9]}) == 9              # the all-zero texts of 0..8 bytes
    assert got[0][0][0] == 0                                 # the empty range


def test_every_flipped_bit_changes_the_crc(checker, tmp_path):
    cases = R.flipped()
    got = check(checker, tmp_path, cases)
    crcs = [g[0][0] for g in got]
    assert len(set(crcs)) == len(crcs)


def test_ranges_outside_the_text_are_refused_without_a_load(checker, tmp_path):
    text = bytes(range(200))
    ranges = [(0, 200), (-1, 4), (0, -1), (197, 4), (201, 0), (200, 0), (0, 201), (1 << 40, 1), (0, 65537)]
    rc, out, got = run(checker, tmp_path, [("outside", text, ranges)])
    assert rc == 0 and CLEAN in out, out
    assert [bad for _, bad in got[0]] == [0, 1, 1, 1, 1, 0, 1, 1, 1]
    assert got[0][0][0] == zlib.crc32(text) and got[0][5][0] == 0


@pytest.mark.parametrize("define, spared", [("-DCRC_START_VALUE=0u", 0), ("-DCRC_FACTOR_OF_LANE(j)=(((j)+1)%64)", 1)])
def test_sensitivity_builds_fail_the_comparison(tmp_path, define, spared):
    """Without the start value EVERY range of the list must differ from zlib: the start value reaches every CRC, an empty
    range's included.  With x^(8 slice (j + 1)) as lane j's factor every range must differ but one: the four bytes 0xFF leave the
    register at zero (they cancel the start value), and zero times any factor is zero."""
    exe = build(tmp_path, define)
    cases = all_cases()
    assert sum(text[o:o + n] == b"\xff" * 4 for _, text, ranges in cases for o, n in ranges) == 1
    rc, out, got = run(exe, tmp_path, cases)
    total = sum(len(c[2]) for c in cases)
    assert rc == 4, out
    assert "%d ranges, 0 refused, 0 loads out of bounds, %d differ from bgzf_crc32, %d differ from zlib.crc32, 0 table" % (
        total, total - spared, total - spared) in out, out
