"""Inputs shared by the CPU model test of the device compressor's lane code (tests/test_bgzf_lane_model.py) and the GPU test of
the kernels (tests/test_gpu_bgzf.py): the smallest shapes at which k_bgzf_deflate can go wrong.  Everything is seeded: the
model's streams of all of them are a fixture (tests/helpers/bgzf_model.py), so a changed input needs it written again."""
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


FIB16 = (1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987, 1597)


def codes_of_15_bits():
    """A member whose literal/length code reaches 15 bits: the whole de Bruijn sequence B(36, 3) over the bytes 48..83 (no
    3-gram twice, about 1,300 of each symbol), then 4,179 units [u v w c] with (u, v, w) distinct triples of the same symbols and
    c one of 16 other bytes with the counts FIB16: nearly every byte is a literal and the rare bytes form a chain in the tree."""
    rng = np.random.default_rng(15)
    head = de_bruijn_prefix(36, 3, 36 ** 3)
    units = sum(FIB16)
    triples = rng.permutation(36 ** 3)[:units]
    c = rng.permutation(np.repeat(np.arange(100, 116), FIB16)).astype(np.uint8)
    body = np.empty((units, 4), np.uint8)
    body[:, 0], body[:, 1], body[:, 2], body[:, 3] = 48 + triples // 1296, 48 + triples // 36 % 36, 48 + triples % 36, c
    return head + body.tobytes()


def length_limit_binds():
    """A member for which bz_build_lengths must halve: 6,763 units [u v c] and no match at all.  (u, v) are distinct pairs of
    150 filler bytes, so no 4-gram comes twice and no 3-gram at a distance of 1..4; c is one of 17 other bytes with the counts
    1, 2, 3, 5, ..., 2584.  With the end-of-block count of 1 these are a Fibonacci chain 16 deep, and the fillers (about 90
    each) only lengthen it.  (A bucket collision could still verify three equal bytes far away; with this seed none does.)"""
    counts, k = [1, 2], 150
    while len(counts) < 17:
        counts.append(counts[-1] + counts[-2])
    rng = np.random.default_rng(7)
    units = sum(counts)
    pairs = rng.permutation(k * k)[:units]
    c = rng.permutation(np.repeat(np.arange(k, k + len(counts)), counts)).astype(np.uint8)
    body = np.empty((units, 3), np.uint8)
    body[:, 0], body[:, 1], body[:, 2] = pairs // k, pairs % k, c
    return body.tobytes()


# byte values per literal/length code length of code_length_limit_binds (the end-of-block symbol is the second of length 15)
CL_LIMIT_SHAPE = {7: 89, 8: 55, 9: 34, 10: 21, 11: 5, 12: 1, 13: 1, 14: 1, 15: 1}


def code_length_limit_binds():
    """A member whose code-length code would be 8 deep without its limit of 7: 32,767 bytes in which a byte value with a
    literal/length code of L bits occurs 2^(15 - L) times (CL_LIMIT_SHAPE: 89 values 256 times each, ... one value once, and the
    end of the block once), so the lengths are forced, and so are the counts of the lengths in the header: 1, 1, 1, 2 (the two
    distance codes), 2, 5, 21, 34, 48 (unused), 55, 89.  The bytes are placed in a seeded order in which no 3-gram comes twice:
    there is no match, and the histogram is exactly this one."""
    rng = np.random.default_rng(77)
    pool, value = [], 0
    for bits, values in CL_LIMIT_SHAPE.items():
        for _ in range(values):
            pool += [value] * (1 << (15 - bits))
            value += 1
    out, seen, waiting = [], set(), []

    def place(s):
        gram = (out[-2], out[-1], s) if len(out) >= 2 else len(out)
        if gram in seen:
            return False
        seen.add(gram)
        out.append(s)
        return True

    for s in rng.permutation(np.asarray(pool, np.int64)).tolist():
        if not place(s):
            waiting.append(s)
        waiting = [w for w in waiting if not place(w)]
    assert not waiting
    return bytes(out)


@functools.lru_cache(None)
def model_inputs():
    """[(name, text)]: the directed members at which the kernel's own parts (the workgroup scan, the LDS atomics, the bit buffer)
    can differ from the host lane model; the precondition of each is asserted on the model by tests/test_bgzf_model_streams.py."""
    rng = np.random.default_rng(4242)
    db = de_bruijn_prefix()
    return [
        # a dynamic block nearly as long as a stored one: the highest words of the bit buffer
        ("buffer_nearly_full", rng.integers(0, 252, DATA).astype(np.uint8).tobytes()),
        ("codes_of_15_bits", codes_of_15_bits()),
        ("length_limit_binds", length_limit_binds()),
        ("code_length_limit_binds", code_length_limit_binds()),
        # hundreds of positions of one step in one bucket; a period below and one above BZ_DIRECT
        ("period2_member", (b"AB" * DATA)[:DATA]),
        ("period5_member", (b"ACGTN" * DATA)[:DATA]),
        # a text without a repeat, then 258 random bytes of other values, then the same 258 again as the member's last bytes
        ("match_258_ends_the_member", db[:1000] + 2 * rng.integers(128, 256, 258).astype(np.uint8).tobytes()),
    ]


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
