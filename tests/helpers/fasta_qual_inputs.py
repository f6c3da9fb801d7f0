"""The inputs of the fasta+qual record stage's tests: the directed cases, the seeded fuzz of valid small texts and the seeded
damage set, shared by tests/test_fasta_qual_lane_model.py (the lane code on the host) and tests/test_gpu_fasta_qual.py (the
kernels).  A case is a dict: name, ftext, qtext, final, max_records, out_cap, max_len, and expect -- None when the device must
take the texts, else (why, which, bad_record) of the hand-back.  want(case) is what fastio.fasta_qual_index makes of it."""
import random

import numpy as np

NON_ASCII, LONE_CR, LINE_TABLE, ROW_CHECK, NAMES, EMPTY, TOKEN, LENGTH, TRUNCATED = 1, 2, 3, 4, 5, 6, 7, 8, 9      # MPB_FQ_WHY_* / MPB_FA_WHY_*
NO_LIMIT = 1 << 40


def render(records, sep=b" ", eol=b"\n", fhdr=None, qhdr=None, last_eol=True):
    """records: (name, sequence, qualities) -> (fasta text, qual text); fhdr / qhdr: what follows the name on the header lines."""
    f, q = [], []
    for name, seq, quals in records:
        f.append(b">" + name + (fhdr or b"") + eol + seq + eol)
        toks = [str(v).encode() if not isinstance(v, bytes) else v for v in quals]
        q.append(b">" + name + (qhdr or b"") + eol + (sep if isinstance(sep, bytes) else b"").join(toks) + eol)
    f, q = b"".join(f), b"".join(q)
    if not last_eol:
        f, q = f[:-len(eol)], q[:-len(eol)]
    return f, q


def case(name, ftext, qtext, final=True, max_records=NO_LIMIT, out_cap=None, max_len=0, expect=None):
    assert len(name) < 32
    return dict(name=name, ftext=bytes(ftext), qtext=bytes(qtext), final=final, max_records=max_records,
                out_cap=2 * len(ftext) + 16 if out_cap is None else out_cap, max_len=max_len, expect=expect)


def want(c):
    """fastio.fasta_qual_index's (out, idx, f_consumed, q_consumed) of a case, or None where the host calls it unsupported."""
    from moira_amd import fastio as F
    rows = min(c["max_records"], len(c["ftext"]) // 2 + 2)
    out, idx = np.zeros(c["out_cap"], np.uint8), np.zeros((rows, 6), np.int64)
    try:
        n, fc, qc, used = F.fasta_qual_index(c["ftext"], c["qtext"], c["final"], rows, out, idx)
    except F.Unsupported:
        return None
    return out[:used], idx[:n], fc, qc


def _good(k, n=4):
    return [(b"r%d" % i, b"ACGTN"[:n] if n <= 5 else b"ACGT" * (n // 4) + b"A" * (n % 4), [(7 * i + j) % 42 for j in range(n)]) for i in range(k)]


def _with(records, at, name=None, seq=None, quals=None):
    r = list(records)
    n0, s0, q0 = r[at]
    r[at] = (n0 if name is None else name, s0 if seq is None else seq, q0 if quals is None else quals)
    return r


def _edit_qual_line(records, at, line):
    """The qual text of `records` with record at's quality line replaced by `line` (bytes, as it stands)."""
    f, q = render(records)
    lines = q.split(b"\n")
    lines[2 * at + 1] = line
    return f, b"\n".join(lines)


def straddle_records():
    """Sixteen records whose quality lines start at every place of a 16-byte word, long enough to cross lane steps and the
    group's 128-byte stride with tokens of one, two and three digits."""
    recs = []
    for k in range(16):
        n = 75 + k
        recs.append((b"s" + b"x" * k, (b"ACGT" * 32)[:n], [(0, 7, 42, 100, 254, 9, 10, 99, 123)[(j + k) % 9] for j in range(n)]))
    return recs


def _tokens_straddle(qtext, every):
    """Whether some multi-digit token of some quality line crosses a multiple of `every` bytes of the text."""
    pos = 0
    for ln in qtext.split(b"\n"):
        if ln and not ln.startswith(b">"):
            at = pos
            for tok in ln.split(b" "):
                if len(tok) > 1 and at // every != (at + len(tok) - 1) // every:
                    return True
                at += len(tok) + 1
        pos += len(ln) + 1
    return False


def directed_cases():
    g = _good(4)
    cs = []
    add = lambda *a, **k: cs.append(case(*a, **k))
    add("digits_1", *render([(b"a", b"ACGTAC", [1, 2, 3, 4, 5, 9])]))
    add("digits_2", *render([(b"a", b"ACGTAC", [10, 25, 38, 41, 77, 99])]))
    add("digits_3", *render([(b"a", b"ACGTAC", [100, 123, 199, 200, 254, 101])]))
    add("digits_mixed", *render([(b"a", b"ACGTACGT", [1, 10, 100, 9, 99, 254, 0, 41])]))
    add("value_0_1_254", *render([(b"a", b"ACG", [0, 1, 254])]))
    add("value_255", *render(_with(g, 2, quals=[1, 255, 3, 4])), expect=(TOKEN, 1, 2))
    add("value_300", *render(_with(g, 1, quals=[300, 2, 3, 4])), expect=(TOKEN, 1, 1))
    add("value_999", *render(_with(g, 3, quals=[1, 2, 3, 999])), expect=(TOKEN, 1, 3))
    add("zeros_007", *render(_with(g, 0, quals=[b"007", b"00", b"010", 4])))                 # three digits: 7, 0, 10
    add("zeros_0007", *render(_with(g, 2, quals=[1, b"0007", 3, 4])), expect=(TOKEN, 1, 2))   # the host reads it; the device does not
    add("tabs", *render(g, sep=b"\t"))
    add("tabs_and_blanks", *_edit_qual_line(g, 1, b"1\t2 3\t4"))
    add("double_blank", *_edit_qual_line(g, 1, b"1  2 3"), expect=(TOKEN, 1, 1))
    add("blank_tab", *_edit_qual_line(g, 3, b"1 \t2 3 4"), expect=(TOKEN, 1, 3))
    add("letter", *_edit_qual_line(g, 2, b"1 a 3 4"), expect=(TOKEN, 1, 2))
    add("minus", *_edit_qual_line(g, 0, b"1 -2 3 4"), expect=(TOKEN, 1, 0))
    add("vertical_tab", *_edit_qual_line(g, 0, b"1 2\x0b3 4"), expect=(TOKEN, 1, 0))
    add("blanks_at_the_ends", *_edit_qual_line(g, 1, b"  1 2 3 4 \t"))
    st = straddle_records()
    f, q = render(st)
    assert _tokens_straddle(q, 16) and _tokens_straddle(q, 128)
    add("straddle", f, q)
    add("one_base", *render([(b"x", b"A", [40])]))
    add("one_base_3_digits", *render([(b"x", b"A", [254])]))
    f, q = render(g)
    add("two_marks", f.replace(b">r1", b">>r1"), q.replace(b">r1", b">>>r1"))
    add("comment_blank", *render(g, fhdr=b" a comment", qhdr=b" another one"))
    add("comment_tab", *render(g, fhdr=b"\tlength=4", qhdr=b" x"))
    add("empty_names", *render([(b"", b"AC", [1, 2]), (b"", b"GT", [3, 4])]))
    add("name_last_byte", f, q.replace(b">r2", b">r7"), expect=(NAMES, 1, 2))
    add("name_length", f, q.replace(b">r1\n", b">r12\n"), expect=(NAMES, 1, 1))
    add("name_is_prefix", f.replace(b">r3\n", b">r3x\n"), q, expect=(NAMES, 1, 3))
    add("crlf", *render(g, eol=b"\r\n"))
    add("lone_cr_fasta", f.replace(b"ACGT\n>r2", b"AC\rGT\n>r2"), q, expect=(LONE_CR, 0, -1))
    add("lone_cr_qual", f, q.replace(b">r2\n", b">r2\r \n"), expect=(LONE_CR, 1, -1))
    add("high_byte_fasta", f.replace(b">r1", b">r\xc3\xa9"), q, expect=(NON_ASCII, 0, -1))
    add("high_byte_qual", f, q.replace(b">r1", b">r\x80"), expect=(NON_ASCII, 1, -1))
    add("not_final", f, q, final=False)
    add("not_final_open_line", *render(g, last_eol=False), final=False)                    # the last record is not complete yet
    add("final_open_line", *render(g, last_eol=False))
    add("final_open_line_crlf", *render(g, eol=b"\r\n", last_eol=False))
    add("odd_lines_fasta", f + b">r4\n", q, expect=(TRUNCATED, 0, -1))
    add("odd_lines_qual", f, q + b">r4\n", expect=(TRUNCATED, 1, -1))
    f3, q3 = render(g[:3])
    add("fewer_in_qual", f, q3, expect=(TRUNCATED, 0, -1))
    add("fewer_in_fasta", f3, q, expect=(TRUNCATED, 1, -1))
    add("fewer_in_qual_not_final", f, q3, final=False)
    add("max_records_cuts", f, q, max_records=3)
    add("max_records_cuts_short_qual", f, q3, max_records=3)                               # (no lines are left over behind the limit's reach)
    add("max_records_0", f, q, max_records=0)
    add("out_cap_cuts", f, q, out_cap=2 * (2 + 2 * 4) + 1)
    add("out_cap_exact", f, q, out_cap=3 * (2 + 2 * 4))
    add("out_cap_0", f, q, out_cap=0)
    add("max_len_3", *render(_good(3, 9)), max_len=3)
    add("empty_sequence", f.replace(b">r1\nACGT\n", b">r1\n\n"), q, expect=(EMPTY, 0, 1))
    add("blank_sequence", f.replace(b">r2\nACGT\n", b">r2\n \t\n"), q, expect=(EMPTY, 0, 2))
    add("empty_quality", *_edit_qual_line(g, 3, b""), expect=(EMPTY, 1, 3))
    add("one_quality_short", *render(_with(g, 1, quals=[1, 2, 3])), expect=(LENGTH, 1, 1))
    add("one_quality_long", *render(_with(g, 2, quals=[1, 2, 3, 4, 5])), expect=(LENGTH, 1, 2))
    add("empty_texts", b"", b"")
    add("empty_texts_not_final", b"", b"", final=False)
    add("blank_line_behind", f + b"\n", q, expect=(TRUNCATED, 0, -1))
    big = [(b"read%04d" % i, (b"ACGTTGCA" * 30)[:200 + i % 37], [(i * 31 + j * 7) % 255 for j in range(200 + i % 37)]) for i in range(110)]
    f, q = render(big)
    assert len(f) > 16384 and f[16384 - 1] != 10 and f[16384] != 10 and q[16384 - 1] != 10 and q[3 * 16384] != 10     # lines over tile edges
    add("tile_edge", f, q)
    add("tile_edge_out_cap", f, q, out_cap=len(f))
    assert len({c["name"] for c in cs}) == len(cs)
    return cs


def long_cases():
    """Records of up to 65535 values (tests/helpers/long_read_inputs.py): both separators, both line ends, an open last line,
    and the refusals beyond byte 200,000 of a quality line."""
    from helpers import long_read_inputs as LR
    return [LR.fasta_qual_case("long_blank_lf"), LR.fasta_qual_case("long_tab_crlf", b"\t", b"\r\n"),
            LR.fasta_qual_case("long_tab_lf_open", b"\t", last_eol=False), LR.fasta_qual_case("long_blank_crlf_max_len", b" ", b"\r\n", max_len=40000),
            LR.fasta_qual_case("long_not_final", final=False)] + LR.fasta_qual_refusals()


_NAME = b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789_:/.-#"


def _valid_text(rng):
    """One valid pair of texts of at most 4 KiB each, with everything the byte-level path allows chosen at random."""
    eol = rng.choice([b"\n", b"\n", b"\r\n"])
    k = rng.randint(1, 6)
    f, q = [], []
    for _ in range(k):
        name = bytes(rng.choice(_NAME) for _ in range(rng.randint(0, 12)))
        n = rng.choice([1, 2, 3, rng.randint(1, 60), rng.randint(30, 60)])
        seq = bytes(rng.choice(b"ACGTNacgtn-.") for _ in range(n))
        kind = rng.randint(0, 3)
        vals = [rng.randint(0, 9) if kind == 0 else rng.randint(10, 99) if kind == 1 else rng.randint(100, 254) if kind == 2
                else rng.choice([rng.randint(0, 254), rng.randint(0, 41)]) for _ in range(n)]
        toks = [(b"%d" % v) if rng.random() < 0.97 else (b"%03d" % v) for v in vals]
        line = b"".join(t + (rng.choice([b" ", b" ", b"\t"]) if i + 1 < n else b"") for i, t in enumerate(toks))
        marks = b">" * rng.choice([1, 1, 1, 2])
        tail = lambda: rng.choice([b"", b"", b" comment", b"\tx=1 y", b" "])
        ends = lambda: rng.choice([b"", b"", b" ", b"\t ", b"  "])
        f.append(marks + name + tail() + eol + ends() + seq + ends() + eol)
        q.append(b">" + name + tail() + eol + ends() + line + ends() + eol)
    return b"".join(f), b"".join(q), k


def fuzz_cases(count=2000, seed=20240611):
    rng = random.Random(seed)
    cs = []
    for i in range(count):
        f, q, k = _valid_text(rng)
        final = rng.random() < 0.6
        if final and rng.random() < 0.3:                      # an unterminated last line
            f, q = f.rstrip(b"\r\n"), q.rstrip(b"\r\n")
            if f.endswith((b" ", b"\t")) or q.endswith((b" ", b"\t")):
                pass                                          # (blanks at the very end: stripped all the same)
        kw = {}
        if rng.random() < 0.25:
            kw["max_records"] = rng.randint(0, k)
        if rng.random() < 0.25:
            kw["out_cap"] = rng.randint(0, 2 * len(f))
        if rng.random() < 0.3:
            kw["max_len"] = rng.randint(1, 40)
        assert len(f) <= 4096 and len(q) <= 4096
        cs.append(case("fuzz%04d" % i, f, q, final=final, **kw))
    return cs


def damage_cases(count=600, seed=977):
    """Valid texts with one byte changed, dropped or added in either text: whatever the host makes of them."""
    rng = random.Random(seed)
    cs = []
    junk = b"0123456789 \t\n\r>aN\x80-\x0b"
    for i in range(count):
        f, q, _ = _valid_text(rng)
        t = [bytearray(f), bytearray(q)]
        for _ in range(rng.choice([1, 1, 2])):
            b = t[rng.randint(0, 1)] if rng.random() < 0.4 else t[1]
            at = rng.randrange(len(b))
            how = rng.randint(0, 2)
            if how == 0:
                b[at] = rng.choice(junk)
            elif how == 1:
                del b[at]
            else:
                b.insert(at, rng.choice(junk))
        cs.append(case("damage%04d" % i, t[0], t[1], final=rng.random() < 0.7))
    return cs
