"""The CRC-32 kernel on the GPU (include/moira_pb.h: mpb_crc32_ranges_host; Engine.crc32_ranges; k_bgzf_crc32).  zlib.crc32 is the
reference, compared with array_equal.  The ranges are tests/helpers/crc_ranges.py's; the same ranges go through the lane code on
the host in tests/test_crc_lane_model.py."""
import zlib

import numpy as np
import pytest

from helpers import crc_ranges as R
from moira_amd import engine as E

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(0)
    yield e
    e.close()


def same_as_zlib(eng, case):
    name, text, ranges = case
    offs = np.array([o for o, _ in ranges], np.int64)
    lens = np.array([n for _, n in ranges], np.int32)
    got = eng.crc32_ranges(text, offs, lens)
    want = np.array([zlib.crc32(text[o:o + n]) for o, n in ranges], np.uint32)
    assert got.dtype == np.uint32 and np.array_equal(got, want), (name, np.flatnonzero(got != want)[:5])
    return got


@pytest.mark.parametrize("tail", [0, 1])
def test_placed_ranges_equal_zlib(eng, tail):
    """Every listed length at the start offsets 0..15 and once ending on the text's last byte; tail = 0: the text's length is 15
    mod 16, so that range ends inside the last, partial 16-byte word."""
    case = R.placed(tail)
    assert (len(case[1]) % 16 == 15) == (tail == 0)
    same_as_zlib(eng, case)


def test_constant_texts(eng):
    zeros, ones = R.constant_texts()
    got = same_as_zlib(eng, zeros)
    assert len(set(got[:9].tolist())) == 9 and got[0] == 0    # nine all-zero texts, nine CRCs; the empty range's is 0
    same_as_zlib(eng, ones)


def test_every_flipped_bit_changes_the_crc(eng):
    cases = R.flipped()
    text = b"".join(c[1] for c in cases)                     # 129 full members in one call
    ranges = [(k * R.RANGE_MAX, R.RANGE_MAX) for k in range(len(cases))]
    got = same_as_zlib(eng, ("flipped", text, ranges))
    assert len(set(got.tolist())) == len(cases)


def test_5000_overlapping_ranges_in_one_call(eng):
    case = R.overlapping(5000)
    assert len(case[2]) == 5000
    same_as_zlib(eng, case)


def test_no_range_and_no_text(eng):
    assert len(eng.crc32_ranges(b"abc", [], [])) == 0
    assert eng.crc32_ranges(b"", [0], [0]).tolist() == [0]
    assert eng.crc32_ranges(b"abc", [3, 0], [0, 3]).tolist() == [0, zlib.crc32(b"abc")]


def test_a_range_past_the_text_is_refused_before_any_launch(eng):
    eng.timing(True)
    eng.timing_reset()
    for offs, lens, k in (([0, 2], [3, 2], 1), ([-1], [1], 0), ([0], [-1], 0), ([4], [0], 0)):
        with pytest.raises(ValueError, match="mpb_crc32_ranges_host: range %d " % k):
            eng.crc32_ranges(b"abc", offs, lens)
    with pytest.raises(ValueError, match="mpb_crc32_ranges_host: range 0 .*longer than 65536"):
        eng.crc32_ranges(bytes(70000), [0], [65537])
    t = eng.kernel_times()
    assert t["bgzf_inflate"][1] == 0, t
    eng.crc32_ranges(b"abc", [0], [3])                       # ... and the kernel's launches are timed under bgzf_inflate
    t = eng.kernel_times()
    eng.timing(False)
    assert t["bgzf_inflate"][1] == 1, t
