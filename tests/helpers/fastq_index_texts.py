"""The directed texts of the device FASTQ indexer's tests (tests/test_fastq_index_lane_model.py runs them through the lane code
on the host, tests/test_gpu_fastq_index.py through the kernels): (name, text, final, max_records) cases.  T is the kernels' tile
(FQ_TILE of moira_amd/csrc/mpb_index_lane.inc)."""
import numpy as np

T = 16384
BIG = 1 << 40          # "no limit" for max_records


def rec(name=b"r", seq=b"ACGT", qual=None, plus=b"+", nl=b"\n"):
    qual = b"I" * len(seq) if qual is None else qual
    return b"@" + name + nl + seq + nl + plus + nl + qual + nl


def records(n, seed=0, lo=1, hi=40, nl=b"\n"):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        m = int(rng.integers(lo, hi + 1))
        seq = bytes(rng.choice(list(b"ACGTN"), m).tolist())
        qual = bytes(rng.integers(33, 74, m).tolist())
        out.append(rec(b"read%d/1 d=%d" % (k, m), seq, qual, nl=nl))
    return out


def fill_to(prefix, size, nl=b"\n"):
    """prefix + whole records, the last one stretched so that the text is exactly `size` bytes and ends with its newline."""
    text = prefix
    while size - len(text) > 200:
        text += rec(b"f", b"ACGTACGTAC", nl=nl)
    left = size - len(text) - len(rec(b"f", b"", b"", nl=nl))
    assert left >= 2
    m, extra = left // 2, left % 2
    return text + rec(b"f" + b"x" * extra, b"A" * m, b"I" * m, nl=nl)


def both(name, text, max_records=BIG):
    return [(name + "/final", text, 1, max_records), (name + "/more", text, 0, max_records)]


def placement():
    """Newline and tile placement."""
    cases = []
    for res in range(16):                                    # the first newline at every residue of 16 (and so the others move too)
        cases += both("residue%d" % res, rec(b"h" * (res + 15)) + b"".join(records(3, res)))
    t = fill_to(b"", T)                                      # a newline as the last byte of a tile, the next line in the next
    cases += both("nl_ends_tile", t + b"".join(records(2, 1)))
    t = fill_to(b"", T + 1)                                  # ... and as the first byte of the next tile
    assert t[T - 1:T + 1] == b"I\n"
    cases += both("nl_first_of_tile", t + b"".join(records(2, 3)))
    for size in (T - 1, T, T + 1):
        cases += both("bytes%d" % size, fill_to(b"", size))
    cases += both("empty", b"")
    cases += both("newlines_only", b"\n" * 37)
    cases += both("newlines_over_a_tile", b"\n" * (T + 5))
    crlf = fill_to(b"", T, nl=b"\r\n")                       # "\r\n" with the "\r" last in a tile
    assert crlf[T - 2:T] == b"\r\n"
    cases += both("cr_ends_tile", b"@" + crlf + b"".join(records(2, 4, nl=b"\r\n")))
    assert (b"@" + crlf)[T - 1:T + 1] == b"\r\n"
    return cases


def endings():
    """End of text, with final 0 and 1."""
    base = b"".join(records(5, 7))
    cases = both("trailing_newline", base) + both("no_trailing_newline", base[:-1])
    for k, extra in enumerate((b"@x\n", b"@x\nAC\n", b"@x\nAC\n+\n"), 1):
        cases += both("lines_beyond%d" % k, base + extra)
        cases += both("lines_beyond%d_open" % k, base + extra[:-1])
    cases += both("partial_last_line", base + b"@x\nAC\n+\nII")
    cases += both("partial_first_line", b"@onl")
    cases += [("cr_last_byte/more", b"".join(records(3, 8, nl=b"\r\n")) + b"@x\r\nAC\r", 0, BIG)]       # must be taken
    cases += both("crlf", b"".join(records(6, 9, nl=b"\r\n")))
    return cases


def limits():
    text = b"".join(records(6, 11))
    return [c for m in (0, 1, 5, 6, 7, 100) for c in both("max_records%d" % m, text, m)]


BAD = {"empty_seq": rec(b"bad", b"", b"II"), "empty_qual": rec(b"bad", b"AC", b""), "mismatch": rec(b"bad", b"ACG", b"II"),
       "blank_seq": rec(b"bad", b" \t", b"II"), "both_empty": rec(b"bad", b"", b"")}


def bad_records():
    good = records(6, 13)
    cases = []
    for kind, bad in BAD.items():
        for where, at in (("first", 0), ("middle", 3), ("last", 6)):
            cases += both("%s_%s" % (kind, where), b"".join(good[:at]) + bad + b"".join(good[at:]))
    cases += both("two_bad", b"".join(good[:2]) + BAD["mismatch"] + good[2] + BAD["empty_seq"] + b"".join(good[3:]))
    cases += both("bad_behind_max_records", b"".join(good[:3]) + BAD["empty_qual"], 3)
    cases += both("bad_at_max_records", b"".join(good[:3]) + BAD["empty_qual"], 4)
    return cases


def headers():
    cases = []
    forms = [b"@id", b"id desc", b"id\tdesc", b"", b" ", b"@", b"@@", b"@ x", b"\tx", b"id  two", b"a@b", b"@id:1:2 x:y"]
    cases += both("header_forms", b"".join(rec(h) for h in forms))
    blanks = b" \t\x0b\x0c\x1c\x1d\x1e\x1f"
    text = b""
    for b in blanks:
        b = bytes([b])
        text += b"@" + b + b"h" + b + b"\n" + b + b"ACGT" + b + b + b"\n" + b + b"+" + b + b"\n" + b + b"IIII" + b + b"\n"
    cases += both("blanks_both_ends", text)
    cases += both("inner_blanks_kept", rec(b"h", b"AC GT", b"II\x0bII"))
    cases += both("all_blank_seq", rec(b"a") + rec(b"h", b" \x0c\x1f ", b"IIII") + rec(b"b"))
    cases += both("all_blank_qual", rec(b"a") + rec(b"h", b"ACGT", b"\t \x1c") + rec(b"b"))
    cases += both("qual_starts_with_at", rec(b"a", b"ACGT", b"@III") + rec(b"b", b"AC", b"@@") + rec(b"c"))
    cases += both("plus_with_content", rec(b"a", plus=b"+a some more") + rec(b"b", plus=b"@not a plus") + rec(b"c", plus=b""))
    return cases


def handed_back():
    """(name, text, final, max_records, why): 1 non-ASCII, 2 lone carriage return."""
    good = records(4, 17)
    cases = []
    for final in (1, 0):
        tag = "/final" if final else "/more"
        cases.append(("lone_cr_in_seq" + tag, good[0] + rec(b"x", b"AC\rGT", b"IIIII") + good[1], final, BIG, 2))
        cases.append(("cr_cr_lf" + tag, good[0] + b"@x\r\r\nAC\nII\n+\n" + good[1], final, BIG, 2))
        cases.append(("non_ascii_header" + tag, good[0] + rec(b"x\xc3\xa9") + good[1], final, BIG, 1))
        cases.append(("non_ascii_0x80" + tag, good[0] + rec(b"x", b"AC\x80T") + good[1], final, BIG, 1))
        cases.append(("lone_cr_behind_bad" + tag, good[0] + BAD["mismatch"] + rec(b"x", b"A\rC", b"III") + good[1], final, BIG, 2))
        cases.append(("non_ascii_behind_bad" + tag, good[0] + BAD["empty_seq"] + rec(b"x\xff") + good[1], final, BIG, 1))
        cases.append(("non_ascii_before_bad" + tag, good[0] + rec(b"x\xff") + BAD["empty_seq"] + good[1], final, BIG, 1))
        cases.append(("lone_cr_behind_max_records" + tag, good[0] + good[1] + rec(b"x", b"A\rC", b"III"), final, 2, 2))
    cases.append(("cr_last_byte/final", b"".join(good) + b"@x\nAC\n+\nII\r", 1, BIG, 2))
    cases.append(("non_ascii_in_open_tail/final", b"".join(good) + b"@x\xfe", 1, BIG, 1))
    return cases


def not_looked_at():
    """Bytes behind the last newline of a non-final text: neither indexer looks at them."""
    good = b"".join(records(4, 19))
    return [("non_ascii_in_open_tail/more", good + b"@x\xfe", 0, BIG), ("lone_cr_in_open_tail/more", good + b"@x\rzz", 0, BIG)]


def long_reads():
    """Records of up to 65535 bases (tests/helpers/long_read_inputs.py: fastq_text), LF and CRLF: whole, cut inside the
    65535-base quality line, and with max_records just before and just behind a long record."""
    from helpers import long_read_inputs as LR
    cases = []
    for tag, nl in (("lf", b"\n"), ("crlf", b"\r\n")):
        text, idx = LR.fastq_text(nl)
        cases += both("long_%s" % tag, text) + both("long_%s_cut_in_quality" % tag, text[:int(idx[1, 4]) + 40000])
        for m in (1, 2, 3, 4):
            cases += both("long_%s_max_records%d" % (tag, m), text, m)
    return cases


def directed():
    return placement() + endings() + limits() + bad_records() + headers() + not_looked_at()


def fuzz(count=2000, seed=2024, most=4096):
    """Texts over ACGTNn@+!I5, blank, tab, "\\n" and "\\r\\n" (no other "\\r", no byte >= 0x80): the host never says unsupported."""
    rng = np.random.default_rng(seed)
    alphabet = [bytes([c]) for c in b"ACGTNn@+!I5 \t"] + [b"\n"] * 4 + [b"\r\n"]
    cases = []
    for k in range(count):
        size = int(rng.integers(0, most)) if k % 8 else int(rng.integers(0, 64))
        picks = rng.integers(0, len(alphabet), size)
        text = b"".join(alphabet[i] for i in picks)[:most]
        if text.endswith(b"\r"):
            text = text[:-1]
        cases.append(("fuzz%d" % k, text, int(rng.integers(0, 2)), BIG if k % 3 else int(rng.integers(0, 20))))
    return cases
