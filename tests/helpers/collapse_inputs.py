"""The cases of the device collapse step (mpb_collapse_text_host; what a lane does: moira_amd/csrc/mpb_collapse_lane.inc), shared
by the host lane model (tests/test_collapse_lane_model.py), the grouped host entry's tests (tests/test_collapse_grouped.py) and the
GPU test (tests/test_gpu_collapse_text.py).  A case is a dict: `name`, `text` (bytes), `idx` (int64[n][6]; only SEQ_OFF and
SEQ_LEN matter to the step), `max_len`, and for the lane model alone `forge` (0: none; 1: every hash[] entry the same value; 2:
hashes that differ between sequences but all start their probe walk at one slot).  The oracle of hash is fastio.py2_hashes, the
oracle of rep a dict of truncated sequences to first index.  Texts made by raw() hold the bare sequences (any byte, any place);
texts made by fastq() are whole FASTQ records a parser takes."""
import gzip
import os

import numpy as np

from moira_amd import fastio as F

GOLD = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden")
LENGTHS = (1, 15, 16, 17, 31, 32, 33, 255, 256, 257)
TABLE_COUNTS = (63, 64, 65, 4095, 4096, 4097)


def raw(seqs, gaps=None, tail=b""):
    """(text, idx) of bare sequences laid behind each other, gaps[i] bytes of '.' in front of sequence i (default 1), `tail` behind."""
    parts, rows, at = [], [], 0
    for i, s in enumerate(seqs):
        g = 1 if gaps is None else gaps[i]
        parts.append(b"." * g + s)
        rows.append((0, 0, at + g, len(s), at + g, len(s)))
        at += g + len(s)
    return b"".join(parts) + tail, np.array(rows, np.int64).reshape(len(seqs), 6)


def fastq(seqs, rng):
    """(text, idx) of FASTQ records with these sequences and seeded qualities; the index by hand, mio_fastq_index's columns."""
    parts, rows, at = [], [], 0
    for i, s in enumerate(seqs):
        head = b"@r%d\n" % i
        q = bytes(rng.integers(35, 74, len(s), dtype=np.uint8).tolist())
        rows.append((at + 1, len(head) - 2, at + len(head), len(s), at + len(head) + len(s) + 3, len(s)))
        rec = head + s + b"\n+\n" + q + b"\n"
        parts.append(rec)
        at += len(rec)
    return b"".join(parts), np.array(rows, np.int64).reshape(len(seqs), 6)


def bases(rng, n):
    return bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].tolist())


def case(name, text, idx, max_len=0, forge=0):
    return dict(name=name, text=bytes(text), idx=np.ascontiguousarray(idx, np.int64).reshape(-1, 6), max_len=max_len, forge=forge)


def sequences(c):
    idx, ml = c["idx"], c["max_len"]
    return [c["text"][int(r[F.SEQ_OFF]):int(r[F.SEQ_OFF]) + (min(int(r[F.SEQ_LEN]), ml) if ml > 0 else int(r[F.SEQ_LEN]))] for r in idx]


def want(c):
    """(hash uint64[n], rep int32[n]) of a case: fastio.py2_hashes, and a dict of truncated sequences to first index."""
    h = np.array(F.py2_hashes(c["text"], c["idx"], c["max_len"]), np.uint64) if len(c["idx"]) else np.zeros(0, np.uint64)
    first, rep = {}, np.zeros(len(c["idx"]), np.int32)
    for k, s in enumerate(sequences(c)):
        rep[k] = first.setdefault(s, k)
    return h, rep


def drawn(name, n, distinct, seed, length=40, max_len=0, whole=False):
    """n records drawn (seeded) from `distinct` different sequences of `length` bases."""
    rng = np.random.default_rng(seed)
    pool = set()
    while len(pool) < distinct:
        pool.add(bases(rng, length))
    pool = sorted(pool)
    seqs = [pool[i] for i in rng.integers(0, distinct, n)]
    return case(name, *(fastq(seqs, rng) if whole else raw(seqs)), max_len=max_len)


def small_cases():
    rng = np.random.default_rng(11)
    out = [case("n0", b"ACGT", np.zeros((0, 6), np.int64)), case("n1", *raw([b"ACGTACGTAC"]))]
    # L = 0: several, at different places (the text's end among them), between records that are not empty
    text, idx = raw([b"", b"ACGT", b"", b"A", b"", b"ACGT", b""])
    idx[6, 2] = idx[6, 4] = len(text)
    out.append(case("empties", text, idx))
    # every length: two equal copies, one that differs in the last byte, one in the first
    seqs = []
    for L in LENGTHS:
        s = bases(rng, L)
        seqs += [s, s[:-1] + b"N", s, b"N" + s[1:], s]
    out.append(case("lengths", *raw(seqs)))
    # every start offset modulo 16: the same 37 bases at every alignment, and a second sequence that differs in byte 36
    s, seqs, gaps, at = bases(rng, 37), [], [], 0
    for a in list(range(16)) + list(range(15, -1, -1)):
        g = (a - at) % 16
        seqs.append(s if len(seqs) % 3 else s[:-1] + b"N")
        gaps.append(g)
        at += g + 37
    text, idx = raw(seqs, gaps)
    assert sorted(set(int(o) % 16 for o in idx[:, 2])) == list(range(16))
    out.append(case("offsets", text, idx))
    # a sequence at byte 0, one that ends at the last byte; a text whose length is no multiple of 16, and one whose length is
    for name, n in (("edges_odd", 22), ("edges_16", 21)):
        s = bases(rng, n)
        text, idx = raw([s, b"GG", s], gaps=[0, 3, 1])
        assert idx[0, 2] == 0 and idx[2, 2] + idx[2, 3] == len(text) and (len(text) % 16 == 0) == (name == "edges_16"), len(text)
        out.append(case(name, text, idx))
    # pairs that differ only in the first byte, the last byte, in case, in length (a prefix)
    s = bases(rng, 50)
    out.append(case("pairs", *raw([s, b"T" + s[1:] if s[:1] != b"T" else b"A" + s[1:], s[:-1] + (b"T" if s[-1:] != b"T" else b"A"), s.lower(),
                                   s[:49], s[:16], s[:17], s + b"A", s, s.lower(), s[:49]])))
    # 0xFF and 0x00 inside a sequence (bytes are unsigned in the hash)
    z = bytes([65, 0xFF, 67, 0x00, 71, 0xFF, 0xFF, 0x00]) * 5
    out.append(case("bytes_ff_00", *raw([z, z[:-1] + b"\x7f", z, bytes([0xFF]), bytes([0x00]), bytes([0xFF]), bytes([0x00, 0x00]), bytes([0x00])])))
    return out


def truncation_cases():
    """Pairs that become equal only under max_len, with max_len on and off."""
    rng = np.random.default_rng(12)
    s = bases(rng, 20)
    seqs = [s + b"ACGTACGT", s + b"TTTTTTTT", s + b"AC", s, s[:19], s[:19] + b"N" + b"ACGTACGT", s + b"ACGTACGT"]
    text, idx = raw(seqs)
    return [case("truncation_on", text, idx, max_len=20), case("truncation_off", text, idx, max_len=0),
            case("truncation_longer", text, idx, max_len=300)]


def count_cases():
    rng = np.random.default_rng(13)
    s = bases(rng, 33)
    out = [case("same_1000", *raw([s] * 1000))]
    out.append(case("distinct_1000", *raw([b"%04d" % i + s for i in range(1000)])))
    for n in TABLE_COUNTS:
        out.append(drawn("table_%d" % n, n, n // 3 + 1, 100 + n, length=24))
    return out


def big_cases(whole=False):
    """20,000 records from 37 and from 15,000 distinct sequences (whole: FASTQ records a Collapse object takes)."""
    return [drawn("few_20000", 20000, 37, 14, whole=whole), drawn("many_20000", 20000, 15000, 15, whole=whole)]


def golden_text():
    with gzip.open(os.path.join(GOLD, "test1.fastq.gz"), "rb") as fh:
        text = fh.read()
    idx, consumed, err = F.index(text, True, 1 << 20)
    assert err is None and consumed == len(text) and len(idx) == 1000
    return text, idx.copy()


def golden_cases():
    text, idx = golden_text()
    return [case("golden", text, idx), case("golden_100", text, idx, max_len=100)]


def py2_hash_np(seqs):
    """CPython 2.7's hash(str) of every row of a uint8 matrix of equally long, non-empty sequences, in numpy (uint64, wrapping)."""
    m, L = seqs.shape
    with np.errstate(over="ignore"):
        x = seqs[:, 0].astype(np.uint64) << np.uint64(7)
        for j in range(L):
            x = (x * np.uint64(1000003)) ^ seqs[:, j].astype(np.uint64)
        x ^= np.uint64(L)
    x[x == np.uint64(0xFFFFFFFFFFFFFFFF)] = np.uint64(0xFFFFFFFFFFFFFFFE)
    return x


def table_of(n):
    """(cap, cap_shift) of n records, ClParams' rule: cap the power of two that is at least max(16, 2 n)."""
    cap = 16
    while cap < 2 * n:
        cap *= 2
    return cap, 64 - (cap.bit_length() - 1)


def start_slots(h, n):
    """cl_start of the hashes h (uint64) in the table of n records."""
    with np.errstate(over="ignore"):
        return ((h * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(table_of(n)[1])).astype(np.int64)


_CANDIDATES = []


def one_slot_sequences(n, slot, distinct, length=24):
    """`distinct` different sequences of `length` bases whose real hash starts its probe walk at `slot` of the table of n records,
    found by seeded search; the hashes are pairwise different and are fastio.py2_hashes'."""
    if not _CANDIDATES:
        pool = np.frombuffer(b"ACGT", np.uint8)[np.random.default_rng(18).integers(0, 4, (1000000, length))]
        _CANDIDATES.append((pool, py2_hash_np(pool)))
    pool, h = _CANDIDATES[0]
    assert pool.shape[1] == length
    hit = np.flatnonzero(start_slots(h, n) == slot)[:distinct]
    assert len(hit) == distinct, (len(hit), distinct)
    seqs = [pool[i].tobytes() for i in hit]
    text, idx = raw(seqs)
    real = np.array(F.py2_hashes(text, idx, 0), np.uint64)
    assert np.array_equal(real, h[hit]) and len(set(real.tolist())) == distinct == len(set(seqs))
    assert (start_slots(real, n) == slot).all()
    return seqs


def crowded_cases():
    """Long probe walks under real hashes, which the GPU can run (forged_cases: the lane model alone): 4,096 records of 64
    sequences that all start at slot cap - 2, so that every walk but the first two wraps around the table's end, and 600 records
    of 200 sequences that all start at slot 0."""
    out = []
    for name, n, distinct, slot, seed in (("crowded_wrap_4096", 4096, 64, table_of(4096)[0] - 2, 19), ("crowded_slot0_600", 600, 200, 0, 20)):
        seqs = one_slot_sequences(n, slot, distinct)
        draw = np.random.default_rng(seed).integers(0, distinct, n)
        draw[:distinct] = np.random.default_rng(seed).permutation(distinct)      # (every sequence is there)
        c = case(name, *raw([seqs[i] for i in draw]))
        assert len(c["idx"]) == n and len(set(start_slots(np.array(F.py2_hashes(c["text"], c["idx"], 0), np.uint64), n).tolist())) == 1
        out.append(c)
    return out


def long_cases():
    """Sequences of 65535 bases (tests/helpers/long_read_inputs.py: collapse_seqs), with max_len 0 and 40000."""
    from helpers import long_read_inputs
    return long_read_inputs.collapse_cases()


def all_cases():
    return small_cases() + truncation_cases() + count_cases() + big_cases() + golden_cases() + crowded_cases()


def forged_cases():
    """For the lane model alone: the group step reads hash[] as an input, so the byte compare is pinned with hashes no text has."""
    rng = np.random.default_rng(16)
    s = bases(rng, 40)
    seqs = [s, s[:-1] + b"N", s, b"N" + s[1:], s[:20] + b"N" + s[21:], s[:-1] + b"N", s[:39], s[:39], s]
    text, idx = raw(seqs)
    many = drawn("x", 600, 200, 17, length=24)
    return [case("forged_equal", text, idx, forge=1), case("forged_equal_600", many["text"], many["idx"], forge=1),
            case("forged_one_slot", text, idx, forge=2), case("forged_one_slot_600", many["text"], many["idx"], forge=2)]


def bad_row_cases():
    """(case, first bad record): a sequence range past the text, a negative offset, a negative length."""
    text, idx = raw([b"ACGT"] * 5)
    out = []
    for name, k, col, v in (("bad_past", 3, 3, len(text)), ("bad_off", 1, 2, -1), ("bad_len", 4, 3, -1), ("bad_off_past", 2, 2, len(text) + 1)):
        i = idx.copy()
        i[k, col] = v
        out.append((case(name, text, i), k))
    return out
