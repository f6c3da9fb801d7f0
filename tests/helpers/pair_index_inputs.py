"""Paired FASTQ texts for the text-alone paired entry (tests/test_gpu_pair_index.py, tests/test_pair_index_consumer.py): the two
mates' files as bytes from helpers.contig_pairs.Pair lists, the golden test1 / test2 texts, and the reference every case is
compared with -- fastio.index x 2 + fastio.first_header_mismatch + a contigs_filter_text on the two indexes cut to the built pairs."""
import bz2
import gzip
import os

import numpy as np

from helpers import contig_pairs as P
from moira_amd import fastio

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
GOLD = os.path.join(ROOT, "tests", "golden")

_cache = {}


def golden_texts():
    """(test1.fastq, test2.fastq) of tests/golden as bytes: 1,000 pairs."""
    if "gold" not in _cache:
        _cache["gold"] = (gzip.open(os.path.join(GOLD, "test1.fastq.gz")).read(), bz2.open(os.path.join(GOLD, "test2.fastq.bz2")).read())
    return _cache["gold"]


def fastq_text(records, eol=b"\n", last_eol=True):
    """[(name bytes, seq bytes, qual bytes)] -> the file's bytes; the header line carries a comment behind the token."""
    out = []
    for k, (name, seq, qual) in enumerate(records):
        out.append(b"@" + name + b" 1:N:0:7" + eol + seq + eol + b"+" + eol + qual + (eol if last_eol or k + 1 < len(records) else b""))
    return b"".join(out)


def pair_texts(pairs, names=None, rnames=None, **kw):
    """The two files of a list of Pairs; names / rnames: the header tokens (default: p<i>, the same in both files)."""
    names = names or [("p%d" % i).encode() for i in range(len(pairs))]
    rnames = rnames or names
    f = fastq_text([(names[i], p.fwd.encode("latin-1"), p.fq) for i, p in enumerate(pairs)], **kw)
    r = fastq_text([(rnames[i], p.rev.encode("latin-1"), p.rq) for i, p in enumerate(pairs)], **kw)
    return f, r


def class_pairs(seed=11, n=600):
    """n pairs of lengths 1..384 that cover all ten LDS size classes (the longest class needs both reads near 384), ACGT reads
    with qualities 2..41 at offset 33: the device takes every one with the default scores."""
    rng = np.random.default_rng(seed)
    edge = (1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 300, 383, 384)
    pairs = []
    for k in range(n):
        if k % 3 == 0:
            l1, l2 = edge[(k // 3) % len(edge)], edge[(k // 3 * 7 + k // 51) % len(edge)]
        else:
            l1, l2 = int(rng.integers(1, 385)), int(rng.integers(1, 385))
        pairs.append(P.make_pair(rng, l1, l2, ("overlap", "unrelated", "contained")[k % 3]))
    return pairs


def reference(eng, ftext, rtext, ffinal=True, rfinal=True, max_records=None, **kw):
    """What the host builds today and the call made from it -> a dict of every output of the text-alone entry.  kw: what
    contigs_filter_text takes (scores, consensus, filter settings)."""
    limit = max_records if max_records is not None else max(len(ftext), len(rtext)) // 4 + 1
    f, r = fastio.index(ftext, ffinal, limit), fastio.index(rtext, rfinal, limit)
    n_pairs = min(len(f[0]), len(r[0]))
    mismatch = fastio.first_header_mismatch(ftext, f[0][:n_pairs], rtext, r[0][:n_pairs]) if n_pairs else -1
    n_built = n_pairs if mismatch < 0 else mismatch
    fc, rc = fastio.index(ftext, ffinal, n_pairs)[1] if n_pairs else 0, fastio.index(rtext, rfinal, n_pairs)[1] if n_pairs else 0
    res = eng.contigs_filter_text(ftext, f[0][:n_built], rtext, r[0][:n_built], **kw) if n_built else None
    return dict(fidx=f[0], ridx=r[0], f_bad=f[2], r_bad=r[2], n_pairs=n_pairs, mismatch=mismatch, n_built=n_built, f_consumed=fc,
                r_consumed=rc, res=res)


def same_error(a, b):
    if a is None or b is None:
        return a is None and b is None
    return (a.kind, a.header) == (b.kind, b.header)


def assert_same(got, want):
    """Engine.contigs_filter_fastq's result against reference()'s, bit for bit on every output (a slot's bytes past
    hdr_len + 2 clen and the values of a handed-back pair are undefined on both sides and are not compared)."""
    assert np.array_equal(got.fidx, want["fidx"]) and np.array_equal(got.ridx, want["ridx"])
    assert same_error(got.f_bad, want["f_bad"]) and same_error(got.r_bad, want["r_bad"])
    assert (got.n_pairs, got.mismatch, got.n_built, got.f_consumed, got.r_consumed) == \
        (want["n_pairs"], want["mismatch"], want["n_built"], want["f_consumed"], want["r_consumed"])
    w = want["res"]
    n = want["n_built"]
    assert len(got.done) == n
    if w is None:
        return
    assert got.rec_cap == w.rec_cap
    assert np.array_equal(got.done, w.done) and (got.n_done, got.n_handed_back) == (w.n_done, w.n_handed_back)
    d = np.nonzero(w.done)[0]
    assert np.array_equal(got.cidx[d], w.cidx[d]) and np.array_equal(got.aux[d], w.aux[d])
    assert P.records(got.cbuf, got.cidx[d]) == P.records(w.cbuf, w.cidx[d])
    assert np.array_equal(got.filtered, w.filtered)
    f = np.nonzero(w.filtered)[0]
    assert np.array_equal(got.ee[f].view(np.uint64), w.ee[f].view(np.uint64))            # bit for bit
    for name in ("ns", "passed", "lens", "has_n"):
        assert np.array_equal(getattr(got, name)[f], getattr(w, name)[f]), name
    assert (got.n_pass, got.n_overflow) == (w.n_pass, w.n_overflow)
    assert (got.filter_error is None) == (w.filter_error is None)
    if w.filter_error is not None:
        assert (str(got.filter_error), got.filter_error.bad_record) == (str(w.filter_error), w.filter_error.bad_record)
