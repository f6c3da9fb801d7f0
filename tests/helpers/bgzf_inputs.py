"""Inputs shared by the CPU model test of the device compressor's lane code (tests/test_bgzf_lane_model.py) and the GPU test of
the kernels (tests/test_gpu_bgzf.py): the smallest shapes at which k_bgzf_deflate can go wrong.  Everything is seeded."""
import functools
import gzip
import os
import struct
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
DATA = 0xff00                 # MPB_BGZF_DATA: text bytes per member
STEP = 256                    # BZ_STEP: positions a workgroup looks up before any of them is inserted
LENGTHS = (0, 1, 2, 3, 4, 257, 258, 259, DATA - 1, DATA, DATA + 1, 2 * DATA + 7)


def fastq_like(rng, n):
    """n bytes that look like FASTQ records: bases over ACGT with repeats between records, quality runs."""
    out = bytearray()
    amplicon = rng.choice(list(b"ACGT"), 250).astype(np.uint8)
    k = 0
    while len(out) < n:
        seq = amplicon.copy()
        flip = rng.integers(0, 250, 6)
        seq[flip] = rng.choice(list(b"ACGT"), 6)
        qual = np.repeat(rng.integers(35, 74, 25).astype(np.uint8), rng.integers(1, 20, 25))[:250]
        qual = np.resize(qual, 250)
        out += b"@M1_%d_%d\n" % (k, int(rng.integers(0, 99999))) + seq.tobytes() + b"\n+\n" + qual.tobytes() + b"\n"
        k += 1
    return bytes(out[:n])


def periodic(rng, period, n, alphabet=256):
    blk = rng.integers(0, alphabet, period).astype(np.uint8).tobytes()
    return (blk * (n // period + 1))[:n]


@functools.lru_cache(None)
def de_bruijn_prefix(k=64, n=3, length=60000):
    """The first `length` symbols of a de Bruijn sequence B(k, n) (concatenated Lyndon words): every n-gram in it is distinct, so
    a text made of it has no repeat of three bytes at all."""
    a = [0] * (k * n)
    seq = []

    def db(t, p):
        if len(seq) >= length:
            return
        if t > n:
            if n % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)
    db(1, 1)
    s = bytes(48 + v for v in seq[:length])
    assert len(s) == length and len({s[i:i + 3] for i in range(length - 2)}) == length - 2
    return s


@functools.lru_cache(None)
def golden_text():
    return gzip.open(os.path.join(ROOT, "tests", "golden", "test1.fastq.gz")).read()


@functools.lru_cache(None)
def golden_renderings():
    """(fastq, fasta, qual) texts of tests/golden/test1.fastq.gz as the CLI writes them (>header / sequence; >header / scores)."""
    lines = golden_text().split(b"\n")
    fasta, qual = [], []
    for k in range(0, len(lines) - 3, 4):
        h, s, q = lines[k][1:], lines[k + 1], lines[k + 3]
        fasta.append(b">" + h + b"\n" + s + b"\n")
        qual.append(b">" + h + b"\n" + b" ".join(b"%d" % (c - 33) for c in q) + b"\n")
    return golden_text(), b"".join(fasta), b"".join(qual)


def fuzz_member(seed):
    """One member of random length, alphabet size 1..256 and repeat structure (copies of earlier stretches at random distances)."""
    rng = np.random.default_rng(1000 + seed)
    n = int(rng.integers(1, DATA + 1))
    alpha = int(rng.integers(1, 257))
    out = bytearray(rng.integers(0, alpha, min(n, int(rng.integers(1, 400)))).astype(np.uint8).tobytes())
    p_copy = float(rng.uniform(0.05, 0.95))
    while len(out) < n:
        if rng.random() < p_copy:
            dist = int(rng.integers(1, min(len(out), 40000) + 1))
            ln = int(rng.integers(3, 600))
            for _ in range(ln):                    # (an overlapping copy when ln > dist)
                out.append(out[-dist])
        else:
            out += rng.integers(0, alpha, int(rng.integers(1, 64))).astype(np.uint8).tobytes()
    return bytes(out[:n])


@functools.lru_cache(None)
def named_inputs():
    """[(name, text)]: every directed input but the golden texts and the fuzz members."""
    rng = np.random.default_rng(42)
    rand_full = rng.integers(0, 256, DATA).astype(np.uint8).tobytes()
    cases = [("len%d" % n, fastq_like(np.random.default_rng(n), n)) for n in LENGTHS]
    cases.append(("one_byte_member", b"I" * DATA))
    for period in (3, 64, STEP - 1, STEP + 1):
        cases.append(("period%d" % period, periodic(rng, period, 5000, 4)))
    cases.append(("period32768", periodic(rng, 32768, DATA)))
    cases.append(("period32769", periodic(rng, 32769, DATA)))
    cases.append(("repeat_across_border", rand_full + rand_full[-500:]))
    cases.append(("random_member", rand_full))
    cases.append(("random_1000", rng.integers(0, 256, 1000).astype(np.uint8).tobytes()))
    cases.append(("all_bytes_twice", bytes(range(256)) * 2))
    cases.append(("no_repeat", de_bruijn_prefix()))
    # the minimum match as the member's last three bytes: a text without a repeat, then three new bytes twice
    cases.append(("min_match_at_end", de_bruijn_prefix()[:700] + b"xyzxyz"))
    return cases


def members(text):
    return [text[k:k + DATA] for k in range(0, len(text), DATA)]


def split_bgzf(blob):
    """[(bsize, deflate bytes, crc, isize)] of a run of BGZF members, every header byte checked."""
    out, pos = [], 0
    while pos < len(blob):
        assert blob[pos:pos + 16] == b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0", pos
        bsize, = struct.unpack_from("<H", blob, pos + 16)
        end = pos + bsize + 1
        assert end <= len(blob)
        crc, isize = struct.unpack_from("<II", blob, end - 8)
        out.append((bsize, blob[pos + 18:end - 8], crc, isize))
        pos = end
    return out


def inflate_raw(stream):
    d = zlib.decompressobj(-15)
    text = d.decompress(stream)
    assert d.eof and not d.unused_data
    return text
