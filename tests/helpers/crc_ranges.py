"""Texts and ranges for the device CRC-32 (k_bgzf_crc32): the host lane model (tests/test_crc_lane_model.py) and the kernel
(tests/test_gpu_crc32.py) see the same list.  A case is (name, text bytes, [(off, len)])."""
import numpy as np

SLICE = 1024                 # CRC_SLICE of moira_amd/csrc/mpb_crc_lane.inc
RANGE_MAX = 65536
LENGTHS = ([0, 1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 31, 32, 33] +
           [SLICE - 1, SLICE, SLICE + 1, 2 * SLICE - 1, 2 * SLICE + 1, RANGE_MAX - 1, RANGE_MAX])


def _random(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def placed(tail=0):
    """Every length at the start offsets 0..15, and once ending on the text's last byte.  The text holds RANGE_MAX + 15 + tail
    bytes: tail = 0 makes its length 15 mod 16, so the last range ends inside the last, partial 16-byte word."""
    text = _random(RANGE_MAX + 15 + tail, 11)
    ranges = [(off, n) for n in LENGTHS for off in range(16)]
    ranges += [(len(text) - n, n) for n in LENGTHS]
    return ("placed/tail%d" % tail, text, ranges)


def constant_texts():
    """All-zero texts of 0..8 bytes (nine distinct CRCs: only the start value carries the length), and all-0xFF texts."""
    zero = bytes(RANGE_MAX)
    ones = b"\xff" * RANGE_MAX
    lens = list(range(9)) + [SLICE, SLICE + 1, RANGE_MAX]
    return [("zeros", zero, [(0, n) for n in lens]), ("ones", ones, [(0, n) for n in lens] + [(3, 4 * SLICE + 5)])]


def flipped():
    """A full member with one bit flipped, at the first and at the last byte of every slice: (name, text, [(0, RANGE_MAX)]).
    The first case is the member itself."""
    base = bytearray(_random(RANGE_MAX, 12))
    out = [("member", bytes(base), [(0, RANGE_MAX)])]
    for j in range(RANGE_MAX // SLICE):
        for at in (j * SLICE, j * SLICE + SLICE - 1):
            t = bytearray(base)
            t[at] ^= 1 << (at % 8)
            out.append(("flip@%d" % at, bytes(t), [(0, RANGE_MAX)]))
    return out


def overlapping(n=5000):
    """n ranges of one text in one call: seeded offsets and lengths, overlapping freely, every 50th a full member."""
    text = _random(3 * RANGE_MAX + 7, 13)
    rng = np.random.default_rng(14)
    ranges = []
    for k in range(n):
        ln = RANGE_MAX if k % 50 == 0 else int(rng.integers(0, 4 * SLICE))
        ranges.append((int(rng.integers(0, len(text) - ln + 1)), ln))
    return ("overlapping", text, ranges)
