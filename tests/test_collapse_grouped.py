"""mio_collapse_add_grouped (fastio.Collapse.add(hash=, rep=)): the same object as mio_collapse_add on the same chunks, from a
hash per record and the first equal record of the chunk -- the oracle's here (tests/helpers/collapse_inputs.py: fastio.py2_hashes
and a dict), the device's in tests/test_gpu_collapse_text.py.  A rep that misses duplicates costs only time; a rep, a hash or a
length that cannot be right is refused before the object is touched; with verify so are a wrong hash and a false duplicate."""
import numpy as np
import pytest

from helpers import collapse_inputs as X
from moira_amd import fastio as F

KINDS = (F.FMT_FASTA, F.FMT_QUAL, F.FMT_FASTQ, F.FMT_NAMES, F.FMT_REPORT)
# chunks of uneven sizes: an empty one, one of one record, and two above the 8,192 records from which the object fills its shards
# on several threads
CUTS = (0, 1, 7, 300, 301, 9001, 19999)


def inputs():
    gt, gi = X.golden_text()
    out = [X.case("golden", gt, gi), X.case("golden_100", gt, gi, max_len=100)] + X.big_cases(whole=True)
    return out


CASES = inputs()


def chunks(c):
    """The case cut into chunks: (idx rows, ee, flags, aux, oracle hash, oracle rep within the chunk)."""
    n = len(c["idx"])
    rng = np.random.default_rng(n)
    ee = np.round(rng.random(n) * 4, 1)                       # (ties among the members of a group: first seen wins)
    flags = (rng.random(n) < 0.1).astype(np.uint8)
    aux = rng.integers(0, 50, (n, 3)).astype(np.int32)
    bounds = sorted(set(min(b, n) for b in CUTS + (n,)))
    out = []
    for lo, hi in zip([0] + bounds, bounds + [n]):
        part = X.case("part", c["text"], c["idx"][lo:hi], max_len=c["max_len"])
        h, rep = X.want(part)
        out.append((part["idx"], ee[lo:hi], flags[lo:hi], aux[lo:hi], h, rep))
    return out


def filled(c, threads, grouped, miss=False):
    g = F.Collapse(threads)
    for idx, ee, flags, aux, h, rep in chunks(c):
        if grouped:
            g.add(c["text"], idx, ee, flags, c["max_len"], aux, hash=h, rep=np.arange(len(idx), dtype=np.int32) if miss else rep)
        else:
            g.add(c["text"], idx, ee, flags, c["max_len"], aux)
    return g


def same_objects(a, b):
    assert len(a) == len(b) > 0
    ea, eb = a.export(), b.export()
    for x, y in zip(ea, eb):
        assert np.array_equal(x, y)
    sel = np.arange(len(a))
    for kind in KINDS:
        for relabel in (None, "Seq"):
            assert bytes(a.format(sel, kind, relabel=relabel)) == bytes(b.format(sel, kind, relabel=relabel)), kind
    return ea


@pytest.mark.parametrize("threads", [1, 16])
@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_the_grouped_entry_makes_the_object_mio_collapse_add_makes(c, threads):
    a, b = filled(c, threads, False), filled(c, threads, True)
    ee, ln, size, _, _ = same_objects(a, b)
    assert len(a) == len(set(X.sequences(c))) and int(size.sum()) == len(c["idx"])
    same_objects(a, filled(c, 1, True))                      # ... and neither depends on the thread count


@pytest.mark.parametrize("threads", [1, 16])
def test_a_rep_that_misses_every_duplicate_costs_only_time(threads):
    for c in CASES[1:3]:
        same_objects(filled(c, threads, False), filled(c, threads, True, miss=True))


def small():
    text, idx = X.fastq([b"ACGTACGT", b"ACGTACGT", b"TTTT", b"ACGTACGT", b"TTTT", b"ACGTACGA", b"ACGA"], np.random.default_rng(1))
    c = X.case("small", text, idx)
    h, rep = X.want(c)
    assert rep.tolist() == [0, 0, 2, 0, 2, 5, 6]
    return c, h, rep


def refused(c, h, rep, what, verify=False):
    g = F.Collapse(1)
    n = len(c["idx"])
    g.add(c["text"], c["idx"][:2], np.zeros(2), np.zeros(2, np.uint8))
    before = (len(g), [bytes(x.tobytes()) for x in g.export()])
    with pytest.raises(ValueError, match=what):
        g.add(c["text"], c["idx"], np.zeros(n), np.zeros(n, np.uint8), hash=h, rep=rep, verify=verify)
    assert (len(g), [bytes(x.tobytes()) for x in g.export()]) == before      # the object is untouched
    g.add(c["text"], c["idx"], np.zeros(n), np.zeros(n, np.uint8))           # ... and works on
    assert len(g) == 4


def test_a_rep_that_cannot_be_right_is_refused_with_the_object_untouched():
    c, h, rep = small()
    forward = rep.copy(); forward[0] = 1
    refused(c, h, forward, "is not in 0")
    negative = rep.copy(); negative[3] = -1
    refused(c, h, negative, "is not in 0")
    chained = rep.copy(); chained[3] = 1                     # record 1 is a duplicate itself
    refused(c, h, chained, "is no representative")
    other = rep.copy(); other[4] = 0                         # TTTT under ACGTACGT: another hash (and another length)
    refused(c, h, other, "differ in hash")
    same_hash = h.copy(); same_hash[4] = same_hash[2] = h[0]
    refused(c, same_hash, other, "differ in length")
    # equal truncated lengths are what counts: under max_len = 4 records 0 and 5 are one sequence, without it they are not
    c4 = X.case("small4", c["text"], c["idx"], max_len=4)
    h4, rep4 = X.want(c4)
    assert rep4.tolist() == [0, 0, 2, 0, 2, 0, 6]
    g = F.Collapse(1)
    g.add(c["text"], c["idx"], np.zeros(7), np.zeros(7, np.uint8), 4, hash=h4, rep=rep4, verify=True)
    assert len(g) == 3
    with pytest.raises(ValueError, match="come together"):
        g.add(c["text"], c["idx"], np.zeros(7), np.zeros(7, np.uint8), hash=h)
    with pytest.raises(ValueError, match="one entry per record"):
        g.add(c["text"], c["idx"], np.zeros(7), np.zeros(7, np.uint8), hash=h[:6], rep=rep[:6])


def test_verify_refuses_a_wrong_hash_and_a_false_duplicate():
    c, h, rep = small()
    wrong = h.copy(); wrong[2] ^= np.uint64(1); wrong[4] ^= np.uint64(1)     # (consistent within its group: only verify sees it)
    refused(c, wrong, rep, r"hash\[2\] is not the sequence's", verify=True)
    # records 0 and 5 differ in their last byte only: same length; with record 0's hash forged onto 5, the checks without verify pass
    false_dup, forged = rep.copy(), h.copy()
    false_dup[5], forged[5] = 0, h[0]
    refused(c, forged, false_dup, "records 5 and 0 of one group differ in sequence", verify=True)
    g = F.Collapse(1)
    g.add(c["text"], c["idx"], np.zeros(7), np.zeros(7, np.uint8), hash=forged, rep=false_dup)     # without verify it is taken: the
    assert len(g) == 3                                                                               # caller's word (the header says so)
    # the same in the smallest chunk there is: two sequences of one length and -- forged -- one hash
    text, idx = X.fastq([b"AAAA", b"AAAT"], np.random.default_rng(2))
    c2 = X.case("two", text, idx)
    h2, _ = X.want(c2)
    with pytest.raises(ValueError, match="records 1 and 0 of one group differ in sequence"):
        F.Collapse(1).add(text, idx, np.zeros(2), np.zeros(2, np.uint8), hash=np.array([h2[0], h2[0]], np.uint64), rep=np.array([0, 0], np.int32), verify=True)
