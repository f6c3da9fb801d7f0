"""The preconditions of tests/helpers/long_read_inputs.py, asserted without a GPU: what the long-read GPU tests
(tests/test_gpu_long_text.py) rely on to reach the paths they are there for, and that the host references take these inputs."""
import numpy as np
import pytest

from helpers import collapse_inputs
from helpers import fasta_qual_inputs
from helpers import long_read_inputs as X
from moira_amd import fastio as F


def test_lengths_hold_every_edge_between_short_neighbours():
    assert X.LONG == (65535, 65534, 32769, 32768, 16385, 16384, 16383, 4097, 4096, 4095, 2049, 2048, 2047, 1025, 1024)
    assert [L for L in X.LENGTHS if L not in X.SHORT] == list(X.LONG) and max(X.LENGTHS) == X.MAX_LEN
    for i, L in enumerate(X.LENGTHS):
        if L in X.LONG:
            assert X.LENGTHS[i - 1] in X.SHORT and X.LENGTHS[i + 1] in X.SHORT
    assert {X.LENGTHS[i - 1] for i, L in enumerate(X.LENGTHS) if L in X.LONG} == set(X.SHORT)


@pytest.mark.parametrize("nl", [b"\n", b"\r\n"], ids=["lf", "crlf"])
@pytest.mark.parametrize("quals", X.QUAL_SETS)
def test_fastq_text_meets_its_preconditions(nl, quals):
    text, idx = X.fastq_text(nl, quals)
    X.check_fastq_text(text, idx, nl)
    quiet, inside, crlf = X.tile_facts(text, idx)
    assert quiet >= 3 and inside == {"header", "sequence", "quality"} and crlf == (nl == b"\r\n")
    qual = np.frombuffer(text, np.uint8)[int(idx[1, F.QUAL_OFF]):int(idx[1, F.QUAL_OFF]) + X.MAX_LEN]
    if quals == "seeded":
        assert qual.min() == 33 + 25 and qual.max() == 33 + 40
    else:
        assert X.every_byte_is_everywhere(text, idx)


def test_the_host_references_take_the_long_records():
    text, idx = X.fastq_text()
    q, lens, flags = F.pack(text, idx, stride=65536)
    assert lens.tolist() == list(X.LENGTHS) and q.shape == (len(idx), 65536) and flags.sum() == 1
    for kind in (F.FMT_FASTA, F.FMT_QUAL, F.FMT_FASTQ):
        assert len(bytes(F.format_records(text, idx, np.arange(len(idx)), kind))) > int(idx[:, F.SEQ_LEN].sum())
    text, idx = X.too_long_text()
    assert idx[2, F.SEQ_LEN] == X.MAX_LEN + 1                # (the host's pack has no such limit: the device entries refuse it)


@pytest.mark.parametrize("sep", [b" ", b"\t"], ids=["blank", "tab"])
@pytest.mark.parametrize("eol", [b"\n", b"\r\n"], ids=["lf", "crlf"])
def test_fasta_qual_texts_meet_their_preconditions(sep, eol):
    f, q = X.fasta_qual_texts(sep, eol)
    for every in (16, 128, X.T):
        assert X.tokens_straddle(q, every, eol)
    c = X.fasta_qual_case("long", sep, eol)
    out, idx, fc, qc = fasta_qual_inputs.want(c)
    assert (fc, qc) == (len(f), len(q)) and idx[:, F.SEQ_LEN].tolist() == list(X.LENGTHS) + [X.MAX_LEN] * 2
    three = out[int(idx[X.THREE_AT, F.QUAL_OFF]):][:X.MAX_LEN]
    one = out[int(idx[X.ONE_AT, F.QUAL_OFF]):][:X.MAX_LEN]
    assert three.min() == 100 and three.max() == 254 and one.min() == 0 and one.max() == 9
    mixed = out[int(idx[1, F.QUAL_OFF]):][:X.MAX_LEN]
    assert min(((mixed < 10).sum(), ((mixed >= 10) & (mixed < 100)).sum(), (mixed >= 100).sum())) > 20000


def test_fasta_qual_refusals_and_the_record_above_the_limit():
    for c in X.fasta_qual_refusals():
        w = fasta_qual_inputs.want(c)
        assert c["expect"][1:] == (1, 1) and (w is None or c["name"] == "long_zeros_0007"), c["name"]    # (the host reads "0007")
    f, q = X.fasta_qual_too_long()
    out, idx, fc, qc = fasta_qual_inputs.want(fasta_qual_inputs.case("too_long", f, q))
    assert len(idx) == 2 and idx[1, F.SEQ_LEN] == idx[1, F.QUAL_LEN] == X.MAX_LEN + 1       # one row, length 65536


def test_collapse_seqs_are_what_they_are_there_for():
    seqs, gaps = X.collapse_seqs()
    s = seqs[0]
    assert len(s) == X.MAX_LEN and len(seqs) == 10
    diff = lambda t: np.flatnonzero(np.frombuffer(t, np.uint8) != np.frombuffer(s, np.uint8)[:len(t)]).tolist() if len(t) <= len(s) else None
    assert [diff(t) for t in seqs[:6]] == [[], [X.MAX_LEN - 1], [], [0], [32768], []]
    whole, cut = X.collapse_cases()
    idx = whole["idx"]
    (at,) = diff(seqs[6])
    start = int(idx[6, F.SEQ_OFF])
    assert (start + at) // 16 == (start + X.MAX_LEN - 1) // 16 and at != X.MAX_LEN - 1     # the last aligned word, not the last byte
    assert seqs[7] == s[:X.MAX_LEN - 1] and seqs[8][:40000] == seqs[9][:40000] == s[:40000] and seqs[8][40000] != seqs[9][40000]
    h, rep = collapse_inputs.want(whole)
    assert rep.tolist() == [0, 1, 0, 3, 4, 0, 6, 7, 8, 9] and len(set(h.tolist())) == 8
    h, rep = collapse_inputs.want(cut)
    assert rep.tolist() == [0, 0, 0, 3, 4, 0, 0, 0, 0, 0] and cut["max_len"] == 40000
    text, fidx = X.collapse_fastq()
    assert np.array_equal(F.index(text, True, 10)[0], fidx) and fidx[:, F.SEQ_LEN].tolist() == [len(t) for t in seqs]
