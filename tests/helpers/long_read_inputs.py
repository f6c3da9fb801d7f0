"""Reads of up to 65535 bases (MPB_MAX_LEN of include/moira_pb.h) for the device text path: the FASTQ index (k_fq_*), k_pack_text,
the fused filter entries, the formatter (k_fmt_*), collapse (k_col_*) and fasta+qual (k_fa_*).  Shared by the GPU tests
(tests/test_gpu_long_text.py, tests/test_gpu_long_text_cli.py), the host lane models (through their own case files) and
tests/test_long_read_inputs.py, which asserts every precondition named here once more without a GPU.  The references are the
host's: fastio.index, fastio.pack, fastio.format_records, fastio.py2_hashes and fastio.fasta_qual_index."""
import functools
import re

import numpy as np

from helpers import collapse_inputs
from helpers import fasta_qual_inputs
from moira_amd import fastio as F

T = 16384                                                    # FQ_TILE: one tile of the index's line kernels
MAX_LEN = 65535                                              # MPB_MAX_LEN
# the edges of MPB_MAX_LEN, of a tile, of the narrow pass's widest row (4096), of the groups' 128-byte step and of a 1024-lane
# scan trip of values
LONG = (65535, 65534, 32769, 32768, 16385, 16384, 16383, 4097, 4096, 4095, 2049, 2048, 2047, 1025, 1024)
SHORT = (1, 300)
LENGTHS = tuple(x for i, L in enumerate(LONG) for x in (SHORT[i % 2], L)) + (SHORT[1],)       # every long record between two short ones
HEADER_LINE = 20000                                          # one record's header line: a token of 300 bytes, a blank, a comment
HEADER_TOKEN = 300
HEADER_AT = LENGTHS.index(32768)
EOL_AT = 2                                                   # this record's header line ends in a tile's last byte
QUAL_SETS = ("seeded", "every")


def bases(rng, n, alphabet=b"ACGT"):
    return np.frombuffer(alphabet, np.uint8)[rng.integers(0, len(alphabet), n)].tobytes()


def every_byte(n, shift=0):
    """n quality bytes that walk 33..126 and move on by one more after every round, so that each of the 94 bytes comes to stand
    at every place modulo 16: one-, two- and three-digit values (at an offset of 0 or 33: 33..126 and 0..93) in every lane."""
    j = np.arange(n, dtype=np.int64) + shift
    return (33 + (j + j // 94) % 94).astype(np.uint8).tobytes()


def tile_facts(text, idx):
    """What the tiles of a text see: (tiles without a newline, line kinds a tile edge falls inside, whether a CR LF pair lies
    across a tile edge)."""
    a = np.frombuffer(text, np.uint8)
    tiles = len(a) // T
    quiet = int(((a[:tiles * T].reshape(tiles, T) == 10).sum(axis=1) == 0).sum())
    edges = np.arange(1, tiles + 1, dtype=np.int64) * T      # an edge e: bytes e - 1 and e lie in different tiles
    inside = set()
    for kind, off, ln in (("header", F.HDR_OFF, None), ("sequence", F.SEQ_OFF, F.SEQ_LEN), ("quality", F.QUAL_OFF, F.QUAL_LEN)):
        lo, hi = idx[:, off], (idx[:, off] + idx[:, ln] if ln is not None else idx[:, F.SEQ_OFF] - 2)     # (the header with its comment)
        if ((edges[None, :] > lo[:, None]) & (edges[None, :] < hi[:, None])).any():
            inside.add(kind)
    crlf = bool(((a[edges[edges < len(a)] - 1] == 13) & (a[edges[edges < len(a)]] == 10)).any())
    return quiet, inside, crlf


@functools.lru_cache(maxsize=None)
def fastq_text(nl=b"\n", quals="seeded"):
    """-> (text, idx): one record per entry of LENGTHS, the index by hand with mio_fastq_index's columns.  Every long record's
    token is sized for a chosen residue modulo 16 of its sequence line; record HEADER_AT has a header line of 20,000 bytes, and
    record EOL_AT a comment sized so that its header line's end (the "\\r" of CRLF) is a tile's last byte.  quals: "seeded"
    (Q25..Q40 at offset 33: a 65535-base read needs few DP rows) or "every" (every byte 33..126 at every place of a lane)."""
    assert quals in QUAL_SETS
    rng = np.random.default_rng(65535)
    parts, rows, at, longs = [], [], 0, 0
    for i, L in enumerate(LENGTHS):
        token, comment = b"r%d_%d" % (i, L), b""
        if i == HEADER_AT:
            token = (token + b"_" + b"t" * HEADER_TOKEN)[:HEADER_TOKEN]
            comment = (b" " + b"a comment; " * (HEADER_LINE // 11 + 1))[:HEADER_LINE - 1 - HEADER_TOKEN]
        elif L in LONG:                                      # the sequence starts at at + 1 + len(token) + len(nl)
            token += b"x" * ((2 + 7 * longs - (at + 1 + len(token) + len(nl))) % 16)
            longs += 1
        if i == EOL_AT:
            assert at + 1 + len(token) + 2 > T
            comment = b" " + b"c" * ((T - 1 - (at + 1 + len(token) + 1)) % T)
        seq = bases(rng, L, b"ACGTN" if L == 4097 else b"ACGT")
        qual = rng.integers(33 + 25, 33 + 41, L, dtype=np.uint8).tobytes()
        if quals == "every":
            qual = every_byte(L, i)
        head = b"@" + token + comment + nl
        mid = nl + b"+" + nl
        rows.append((at + 1, len(token), at + len(head), L, at + len(head) + L + len(mid), L))
        rec = head + seq + mid + qual + nl
        parts.append(rec)
        at += len(rec)
    text, idx = b"".join(parts), np.array(rows, np.int64).reshape(len(LENGTHS), 6)
    check_fastq_text(text, idx, nl)
    return text, idx


def check_fastq_text(text, idx, nl):
    """The preconditions of fastq_text."""
    got, consumed, bad = F.index(text, True, len(idx))
    assert bad is None and consumed == len(text) and np.array_equal(got, idx)                 # (the parser's index is this one)
    assert idx[:, F.SEQ_LEN].tolist() == list(LENGTHS) and np.array_equal(idx[:, F.SEQ_LEN], idx[:, F.QUAL_LEN])
    long_rows = idx[idx[:, F.SEQ_LEN] >= 1024]
    assert len(long_rows) == len(LONG)
    assert len(set((long_rows[:, F.SEQ_OFF] % 16).tolist())) >= 8 and len(set((long_rows[:, F.QUAL_OFF] % 16).tolist())) >= 8
    h = idx[HEADER_AT]
    line_end = text.index(nl, int(h[F.HDR_OFF]))
    assert line_end - int(h[F.HDR_OFF]) + 1 == HEADER_LINE and h[F.HDR_LEN] == HEADER_TOKEN
    assert text[int(h[F.HDR_OFF]) + HEADER_TOKEN:][:1] == b" "
    quiet, inside, crlf = tile_facts(text, idx)
    assert quiet >= 3 and inside == {"header", "sequence", "quality"}, (quiet, inside)
    e = text.index(nl, int(idx[EOL_AT, F.HDR_OFF]))
    assert e % T == T - 1                                    # a line's end in a tile's last byte ...
    assert crlf == (nl == b"\r\n")                           # ... which with CRLF puts "\r" and "\n" into different tiles


def every_byte_is_everywhere(text, idx):
    """Whether the longest record's quality line holds every byte 33..126 at every place modulo 16 of the text."""
    r = idx[int(np.argmax(idx[:, F.QUAL_LEN]))]
    q = np.frombuffer(text, np.uint8)[int(r[F.QUAL_OFF]):int(r[F.QUAL_OFF] + r[F.QUAL_LEN])].astype(np.int64)
    place = (np.arange(len(q)) + int(r[F.QUAL_OFF])) % 16
    return len(set((q * 16 + place).tolist())) == 94 * 16 and q.min() == 33 and q.max() == 126


def too_long_text(nl=b"\n"):
    """Three records a parser takes, the third of 65536 bases -> (text, idx)."""
    rng = np.random.default_rng(65536)
    parts, rows, at = [], [], 0
    for i, L in enumerate((300, 4096, MAX_LEN + 1)):
        head = b"@long%d" % i + nl
        rows.append((at + 1, len(head) - 1 - len(nl), at + len(head), L, at + len(head) + L + 2 * len(nl) + 1, L))
        parts.append(head + bases(rng, L) + nl + b"+" + nl + rng.integers(58, 74, L, dtype=np.uint8).tobytes() + nl)
        at += len(parts[-1])
    text, idx = b"".join(parts), np.array(rows, np.int64)
    assert np.array_equal(F.index(text, True, 3)[0], idx)
    return text, idx


# ---- fasta + qual -----------------------------------------------------------------------------------------------------------------

_TOK = [b"%d" % v for v in range(256)]
THREE_AT = len(LENGTHS)                                      # the record of three-digit values alone: the longest quality line
ONE_AT = THREE_AT + 1


@functools.lru_cache(maxsize=None)
def fasta_qual_records():
    """(name, sequence, quality tokens) per entry of LENGTHS, values drawn (seeded) from 0..9, 10..99 and 100..254 in equal
    parts, then 65535 three-digit values and 65535 one-digit values."""
    rng = np.random.default_rng(254)
    recs = []
    for i, L in enumerate(LENGTHS):
        cls = rng.integers(0, 3, L)
        v = np.where(cls == 0, rng.integers(0, 10, L), np.where(cls == 1, rng.integers(10, 100, L), rng.integers(100, 255, L)))
        recs.append((b"q%d_%d" % (i, L), bases(rng, L), [_TOK[x] for x in v.tolist()]))
    recs.append((b"three", bases(rng, MAX_LEN), [_TOK[x] for x in rng.integers(100, 255, MAX_LEN).tolist()]))
    recs.append((b"one", bases(rng, MAX_LEN), [_TOK[x] for x in rng.integers(0, 10, MAX_LEN).tolist()]))
    assert len(recs) == ONE_AT + 1
    return recs


def tokens_straddle(qtext, every, eol=b"\n"):
    """fasta_qual_inputs._tokens_straddle for any separator and line end: whether some token of two or three digits of some
    quality line crosses a multiple of `every` bytes of the text."""
    pos = 0
    for ln in qtext.split(eol):
        if ln and not ln.startswith(b">"):
            for m in re.finditer(rb"\d{2,}", ln):
                if (pos + m.start()) // every != (pos + m.end() - 1) // every:
                    return True
        pos += len(ln) + len(eol)
    return False


@functools.lru_cache(maxsize=None)
def fasta_qual_texts(sep=b" ", eol=b"\n", last_eol=True):
    """-> (fasta text, qual text) of fasta_qual_records() through fasta_qual_inputs.render."""
    assert sep in (b" ", b"\t")
    f, q = fasta_qual_inputs.render(fasta_qual_records(), sep=sep, eol=eol, last_eol=last_eol)
    lines = q.split(eol)
    assert max(len(ln) for ln in lines) == len(lines[2 * THREE_AT + 1]) == 4 * MAX_LEN - 1 > 256000      # about 256 KiB
    for every in (16, 128, T):
        assert tokens_straddle(q, every, eol), every
        assert sep != b" " or eol != b"\n" or fasta_qual_inputs._tokens_straddle(q, every), every
    return f, q


def fasta_qual_case(name, sep=b" ", eol=b"\n", last_eol=True, **kw):
    f, q = fasta_qual_texts(sep, eol, last_eol)
    return fasta_qual_inputs.case(name, f, q, **kw)


def fasta_qual_refusals():
    """The record of three-digit values alone with one token damaged beyond byte 200,000 of its line (the records in front of it
    left out but one): cases with expect = (TOKEN | LENGTH, 1, 1)."""
    recs = fasta_qual_records()
    name, seq, toks = recs[THREE_AT]
    k = 52000                                                # 4 bytes a token: byte 208,000 of the line
    out = []
    for what, new, why in (("value_255", [b"255"], fasta_qual_inputs.TOKEN), ("zeros_0007", [b"0007"], fasta_qual_inputs.TOKEN),
                           ("double_blank", [b"", toks[k]], fasta_qual_inputs.TOKEN), ("value_dropped", [], fasta_qual_inputs.LENGTH)):
        t = toks[:k] + new + toks[k + 1:]
        f, q = fasta_qual_inputs.render([recs[1], (name, seq, t), recs[2]])
        line = q.split(b"\n")[3]
        assert len(line) > 250000 and sum(len(x) + 1 for x in t[:k]) > 200000
        out.append(fasta_qual_inputs.case("long_" + what, f, q, expect=(why, 1, 1)))
    return out


def fasta_qual_too_long():
    """A record of 65536 bases and values behind a short one -> (fasta text, qual text)."""
    rng = np.random.default_rng(65537)
    L = MAX_LEN + 1
    return fasta_qual_inputs.render([(b"a", b"ACGT", [1, 22, 133, 4]), (b"b", bases(rng, L), [_TOK[x] for x in rng.integers(25, 41, L).tolist()])])


# ---- collapse ---------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def collapse_seqs():
    """-> (sequences, gaps): over a seeded 65535-base sequence s -- s three times at three alignments modulo 16, s with only the
    last, only the first, only byte 32768 changed, s with a byte of its last aligned 16-byte word changed, s[:65534], and two
    sequences that agree in their first 40,000 bytes only (equal under max_len 40000 alone)."""
    rng = np.random.default_rng(40000)
    s = bases(rng, MAX_LEN)
    flip = lambda t, at: t[:at] + (b"A" if t[at:at + 1] != b"A" else b"C") + t[at + 1:]
    tail_a, tail_b = bases(rng, 10000), bases(rng, 10000)
    assert tail_a[0] != tail_b[0]
    seqs = [s, flip(s, MAX_LEN - 1), s, flip(s, 0), flip(s, 32768), s, None, s[:MAX_LEN - 1], s[:40000] + tail_a, s[:40000] + tail_b]
    gaps, at = [], 0
    for k, t in enumerate(seqs):
        g = 1 + (5 * k - (at + 1)) % 16                      # sequence k starts at residue 5 k modulo 16
        gaps.append(g)
        if t is None:                                        # the last aligned word of this copy: bytes word .. end, at least two
            start = at + g
            word = (start + MAX_LEN - 1) // 16 * 16
            assert start + MAX_LEN - word >= 2
            seqs[k] = t = flip(s, word - start)
        at += g + len(t)
    return tuple(seqs), tuple(gaps)


def collapse_cases():
    """The sequences of collapse_seqs() laid out bare (collapse_inputs.raw), with max_len 0 and 40000."""
    seqs, gaps = collapse_seqs()
    text, idx = collapse_inputs.raw(list(seqs), list(gaps))
    copies = [k for k, t in enumerate(seqs) if t == seqs[0]]
    assert len(copies) == 3 and len({int(idx[k, F.SEQ_OFF]) % 16 for k in copies}) == 3
    assert len(set(seqs)) == len(seqs) - 2 and len({t[:40000] for t in seqs}) == 3
    return [collapse_inputs.case("long_65535", text, idx), collapse_inputs.case("long_65535_max_len_40000", text, idx, max_len=40000)]


def collapse_fastq():
    """The same sequences as FASTQ records a parser takes (qualities Q25..Q40) -> (text, idx)."""
    from helpers import format_inputs
    rng = np.random.default_rng(40001)
    seqs, _ = collapse_seqs()
    return format_inputs.build([(b"c%d" % k, t, rng.integers(58, 74, len(t), dtype=np.uint8).tobytes()) for k, t in enumerate(seqs)])
