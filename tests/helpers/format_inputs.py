"""The cases of the output formatter (mpb_format_text_host; what a lane does: moira_amd/csrc/mpb_format_lane.inc), shared by the
host lane model (tests/test_format_lane_model.py) and the GPU tests (tests/test_gpu_format_text.py).  A case is a dict of
fastio.format_records' arguments (`text`, `idx`, `sel` -- None: every record -- and the keywords in `kw`); the reference of every
case is fastio.format_records on the same arguments.  The texts are made by hand with their index beside them, so that rows may
hold what a FASTQ parser would refuse (empty lines, any quality byte); where a parser takes the text, index() agrees."""
import gzip
import os

import numpy as np

from moira_amd import fastio as F

GOLD = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden")
KINDS = (F.FMT_FASTA, F.FMT_QUAL, F.FMT_FASTQ)
KIND_NAME = {F.FMT_FASTA: "fasta", F.FMT_QUAL: "qual", F.FMT_FASTQ: "fastq"}
SEQ_LENGTHS = (0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 300)
TOKEN_LENGTHS = (1, 15, 16, 17, 300)
COUNTS = (0, 1, 63, 64, 65, 255, 256, 257, 1025)          # 1025: one more than one trip of k_fmt_scan
RELABEL_INDEXES = (0, 9, 10, 99, 100, 1 << 31, 10 ** 18)
LABELS = [("l%d_" % i + "x" * 300)[:max(2, 17 * i)] for i in range(16)]   # 2 .. 255 bytes


def build(records, eol=b"\n"):
    """(text, idx) of records (token, seq, qual) laid out as FASTQ; the index by hand, mio_fastq_index's columns."""
    parts, rows, at = [], [], 0
    for token, seq, qual in records:
        assert len(seq) == len(qual)
        head = b"@" + token + eol
        mid = eol + b"+" + eol
        rows.append((at + 1, len(token), at + len(head), len(seq), at + len(head) + len(seq) + len(mid), len(qual)))
        rec = head + seq + mid + qual + eol
        parts.append(rec)
        at += len(rec)
    return b"".join(parts), np.array(rows, np.int64).reshape(len(records), 6)


def token(i, length, colons=False):
    """A header token of exactly `length` bytes."""
    base = b":x%d:" % i + b"ab:c" * 80 if colons else b"%d" % (i % 10) + b"_abcd" * 80
    return base[:length]


def quals(rng, n, lo=33, hi=74):
    return bytes(rng.integers(lo, hi, n, dtype=np.uint8).tolist())


def bases(rng, n):
    return bytes(np.frombuffer(b"ACGTN", np.uint8)[rng.integers(0, 5, n)].tolist())


def case(name, text, idx, sel=None, **kw):
    kw.setdefault("kind", F.FMT_FASTQ)
    return dict(name=name, text=text, idx=np.ascontiguousarray(idx, np.int64), sel=None if sel is None else np.ascontiguousarray(sel, np.int64),
                kw=kw)


def want(c):
    """fastio.format_records on the case's arguments."""
    sel = np.arange(len(c["idx"]), dtype=np.int64) if c["sel"] is None else c["sel"]
    return bytes(F.format_records(c["text"], c["idx"], sel, **c["kw"]))


def length_cases():
    """Every sequence length with every token length, with and without ':', in all kinds (length 0: rows no parser makes)."""
    rng = np.random.default_rng(5)
    recs = [(token(i * 100 + j, tl, colons), bases(rng, sl), quals(rng, sl))
            for i, sl in enumerate(SEQ_LENGTHS) for j, (tl, colons) in enumerate((t, c) for t in TOKEN_LENGTHS for c in (False, True))]
    text, idx = build(recs)
    return [case("lengths_%s" % KIND_NAME[k], text, idx, kind=k) for k in KINDS]


def alignment_cases():
    """Every pair of alignments modulo 16 of the sequence and the quality line: 16 token lengths times 16 sequence lengths."""
    rng = np.random.default_rng(6)
    recs, at = [], 0
    for a in range(16):
        for b in range(16):
            tl = 16 + (a - at - 2) % 16                     # the sequence starts at at + tl + 2
            sl = 20 + (b - a - 3) % 16                      # the qualities start sl + 3 bytes behind it
            recs.append((token(len(recs), tl), bases(rng, sl), quals(rng, sl)))
            at += 1 + tl + 1 + sl + 3 + sl + 1
    text, idx = build(recs)
    assert len({(int(r[2]) % 16, int(r[4]) % 16) for r in idx}) == 256
    return [case("align_%s" % KIND_NAME[k], text, idx, kind=k) for k in KINDS]


def crlf_cases():
    rng = np.random.default_rng(7)
    recs = [(token(i, 5 + i % 20, i % 2 == 1), bases(rng, 30 + 7 * i), quals(rng, 30 + 7 * i)) for i in range(40)]
    text, idx = build(recs, b"\r\n")
    got = F.index(text, True, 40)[0]
    assert np.array_equal(got, idx)                          # (the parser's index of CRLF text is this one)
    return [case("crlf_%s" % KIND_NAME[k], text, idx, kind=k) for k in KINDS]


def count_text(n, seed=8):
    rng = np.random.default_rng(seed)
    recs = [(token(i, 6 + i % 13), bases(rng, 1 + (i * 7) % 40), quals(rng, 1 + (i * 7) % 40)) for i in range(n)]
    return build(recs)


def count_cases():
    out = []
    for n in COUNTS:
        text, idx = count_text(n)
        for k in (KINDS if n in (0, 1, 257, 1025) else (F.FMT_QUAL,)):
            out.append(case("count_%d_%s" % (n, KIND_NAME[k]), text, idx, kind=k))
    return out


def sel_cases():
    text, idx = count_text(100, 9)
    n = len(idx)
    rng = np.random.default_rng(10)
    sels = dict(none=None, reversed=np.arange(n)[::-1], repeats=rng.integers(0, n, 300), subset=np.arange(3, n, 7),
                one=np.array([n - 1]), empty=np.zeros(0, np.int64))
    return [case("sel_%s_%s" % (name, KIND_NAME[k]), text, idx, sel=s, kind=k) for name, s in sels.items() for k in KINDS]


def quality_cases():
    """Quality bytes that give q = -1, 0, 1, 9, 10, 99, 100, 254, 255 and above at fastq_offset 0, 33 and 64 (as far as a byte
    can), in runs long enough to cross a lane's 16 values, with every offset pair of the issue and clamp_q0 on and off."""
    out = []
    for off in (0, 33, 64):
        qs = [q for q in (-1, 0, 1, 9, 10, 99, 100, 254, 255, 256, 300) if 0 <= q + off <= 255] + [255 - off]
        qual = bytes([q + off for q in qs] * 13)            # every value at every place of a lane's word and of a step
        recs = [(b"q%d" % i, b"A" * n, (qual * 3)[i:i + n]) for i, n in enumerate((1, 2, 16, 17, len(qual), 2 * len(qual), 129, 300))]
        text, idx = build(recs)
        for out_off in sorted({off, {0: 33, 33: 64, 64: 33}[off]}):
            for clamp in (True, False):
                for k in (F.FMT_QUAL, F.FMT_FASTQ):
                    out.append(case("q_%d_%d_%d_%s" % (off, out_off, clamp, KIND_NAME[k]), text, idx, kind=k, fastq_offset=off,
                                    out_offset=out_off, clamp_q0=clamp))
    return out


def max_len_cases():
    rng = np.random.default_rng(11)
    recs = [(token(i, 9), bases(rng, 100), quals(rng, 100)) for i in range(5)] + [(b"short", bases(rng, 20), quals(rng, 20))]
    text, idx = build(recs)
    return [case("max_len_%d_%s" % (m, KIND_NAME[k]), text, idx, kind=k, max_len=m) for m in (0, 1, 17, 99, 100, 101, 5000) for k in KINDS]


def relabel_cases():
    """relabel with every index of the issue, and every label id and -1, mixed; relabel and a label of 255 bytes."""
    text, idx = count_text(len(RELABEL_INDEXES) * 6, 12)
    n = len(idx)
    ri = np.array([RELABEL_INDEXES[i % len(RELABEL_INDEXES)] for i in range(n)], np.int64)
    ri[-1] = (1 << 63) - 1                                   # 19 digits
    lab = np.array([(i % 17) - 1 for i in range(n)], np.int32)
    out = []
    for k in KINDS:
        out.append(case("relabel_%s" % KIND_NAME[k], text, idx, kind=k, relabel="Seq_", relabel_index=ri))
        out.append(case("relabel_empty_%s" % KIND_NAME[k], text, idx, kind=k, relabel="", relabel_index=ri))
        out.append(case("relabel_255_%s" % KIND_NAME[k], text, idx, kind=k, relabel="R" * 255, relabel_index=ri))
        out.append(case("labels_%s" % KIND_NAME[k], text, idx, kind=k, labels=LABELS, label_id=lab))
        out.append(case("relabel_labels_%s" % KIND_NAME[k], text, idx, sel=np.arange(n)[::-1], kind=k, relabel="x", relabel_index=ri,
                        labels=LABELS, label_id=lab))
    return out


def golden_text(records=None):
    text = gzip.open(os.path.join(GOLD, "test1.fastq.gz"), "rb").read()
    if records is None:
        return text
    return b"\n".join(text.split(b"\n")[:4 * records]) + b"\n"


def golden_cases():
    """The reference's 1,000 golden reads, in all kinds, as the CLI writes them (truncated and relabelled too)."""
    text = golden_text()
    idx = F.index(text, True, 1 << 20)[0].copy()
    assert len(idx) == 1000
    out = [case("golden_%s" % KIND_NAME[k], text, idx, kind=k) for k in KINDS]
    out.append(case("golden_cli_fastq", text, idx, kind=F.FMT_FASTQ, max_len=150, relabel="Seq", relabel_index=np.arange(1000), clamp_q0=True))
    return out


def long_cases():
    """Records of up to 65535 bases (tests/helpers/long_read_inputs.py: fastq_text): all kinds, truncated inside a lane step,
    reversed with repeats, CRLF, and every quality byte 33..126 at every lane with every offset pair and clamp_q0 on and off."""
    from helpers import long_read_inputs as LR
    text, idx = LR.fastq_text()
    n = len(idx)
    out = [case("long_%s" % KIND_NAME[k], text, idx, kind=k) for k in KINDS]
    out += [case("long_max_len_40000_%s" % KIND_NAME[k], text, idx, kind=k, max_len=40000) for k in KINDS]
    out.append(case("long_reversed_repeats_qual", text, idx, sel=np.concatenate([np.arange(n)[::-1], [1, 1, 3, 0, 1]]), kind=F.FMT_QUAL))
    out.append(case("long_crlf_fastq", *LR.fastq_text(b"\r\n"), kind=F.FMT_FASTQ))
    text, idx = LR.fastq_text(b"\n", "every")
    for off, out_off in ((33, 33), (33, 64), (64, 33)):
        for clamp in (True, False):
            for k in (F.FMT_QUAL, F.FMT_FASTQ):
                out.append(case("long_q_%d_%d_%d_%s" % (off, out_off, clamp, KIND_NAME[k]), text, idx, kind=k, fastq_offset=off,
                                out_offset=out_off, clamp_q0=clamp))
    return out


def all_cases():
    return (length_cases() + alignment_cases() + crlf_cases() + count_cases() + sel_cases() + quality_cases() + max_len_cases() +
            relabel_cases() + golden_cases())


def damaged_cases():
    """(case, the first bad k): rows, sel, relabel_index and label_id that every check must refuse before a byte is read."""
    text, idx = count_text(50, 13)
    n, T = len(idx), len(text)
    out = []

    def add(name, row, col, value, bad=None, **kw):
        a = idx.copy()
        a[row, col] = value
        kw.setdefault("kind", F.FMT_FASTQ)
        out.append((case(name, text, a, **kw), row if bad is None else bad))
    add("hdr_off_past", 20, 0, T + 5)
    add("hdr_one_past", 49, 0, T - int(idx[49, 1]) + 1)
    add("seq_off_past", 20, 2, T + 1)
    add("seq_off_neg", 20, 2, -1)
    add("seq_len_neg", 20, 3, -4)
    add("seq_len_huge", 20, 3, 1 << 40)
    add("qual_off_past", 20, 4, T)
    add("qual_one_past", 49, 4, T - int(idx[49, 3]) + 1)
    add("qual_off_huge", 20, 4, (1 << 63) - 1)
    add("len_mismatch", 20, 5, int(idx[20, 5]) + 1)
    add("len_mismatch_qual", 20, 5, int(idx[20, 5]) - 1, kind=F.FMT_QUAL)
    add("hdr_len_neg", 20, 1, -1, kind=F.FMT_FASTA)
    add("first_of_two", 7, 2, -1, bad=7)
    out[-1][0]["idx"][30, 2] = -1
    sel = np.arange(n)
    for name, v in (("sel_n", n), ("sel_neg", -1), ("sel_huge", 1 << 62)):
        s = sel.copy()
        s[11] = v
        out.append((case(name, text, idx, sel=s), 11))
    ri = np.arange(n)
    ri[33] = -1
    out.append((case("relabel_index_neg", text, idx, relabel="S", relabel_index=ri), 33))
    lab = np.zeros(n, np.int32)
    lab[4] = 3
    out.append((case("label_id_past", text, idx, labels=LABELS[:3], label_id=lab), 4))
    return out


def fasta_ignores_quality_columns():
    """FASTA reads no quality: rows whose quality columns hold anything are taken (the contigs' index has its own there)."""
    text, idx = count_text(20, 14)
    a = idx.copy()
    a[:, 4] = -7
    a[:, 5] = 1 << 50
    return case("fasta_any_quality_columns", text, a, kind=F.FMT_FASTA)
