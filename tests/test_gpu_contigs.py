"""k_contig on the GPU, through the C ABI (include/moira_pb.h: mpb_contigs_text_host; Engine.contigs_text,
moira_amd.contig.contigs_from_fastq(engine=...), the CLI's --device_contigs).  The contract is byte identity with the host
library (mct_nw_align, mct_contigs_from_fastq), which tests/test_contig.py pins to the reference's fixtures; the fixtures
(nw_pairs / nw_contigs, and nw_domain: the edges of the domain) are also run here directly.  A slot's bytes past
hdr_len + 2 clen are undefined on both sides and are not compared.
The per-lane code on the host, with checked loads and damaged descriptors: tests/test_contig_device_model.py."""
import os

import numpy as np
import pytest

from helpers import contig_pairs as P
from moira_amd import cli
from moira_amd import contig as CT
from moira_amd import engine as E

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
EDGE = (1, 2, 3, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 300, 301, 383, 384)
KINDS = ("overlap", "ties", "unrelated", "contained", "identical")
SETTINGS = ((1, -1, -2), (2, -3, -1), (1, 0, 0))


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(0)
    yield e
    e.close()


def device(eng, pairs, prm=(1, -1, -2), insert=20, deltaq=6, mode="best", cap=40, trim=False, offset=33, alignments=True):
    fbuf, fidx, rbuf, ridx = P.texts(pairs)
    r = eng.contigs_text(fbuf, fidx, rbuf, ridx, offset, prm[0], prm[1], prm[2], insert, deltaq, P.MODES[mode], cap, trim,
                         alignments=alignments)
    return (fbuf, fidx, rbuf, ridx), r


def alignment_of(r, i):
    n = int(r.aln_len[i])
    return r.aln[i, 0, :n].tobytes().decode("latin-1"), r.aln[i, 1, :n].tobytes().decode("latin-1"), int(r.score[i])


def assert_equals_host(eng, pairs, prm=(1, -1, -2), insert=20, deltaq=6, mode="best", cap=40, trim=False, offset=33, expect_done=None):
    """Alignment strings and scores against mct_nw_align, slots / index rows / aux rows against mct_contigs_from_fastq, for every
    pair the device built; done against expect_done (default: all built)."""
    texts, r = device(eng, pairs, prm, insert, deltaq, mode, cap, trim, offset)
    want_done = np.ones(len(pairs), bool) if expect_done is None else np.asarray(expect_done, bool)
    assert r.done.tolist() == want_done.tolist()
    assert (r.n_done, r.n_handed_back) == (int(want_done.sum()), int((~want_done).sum()))
    built = [p for p, d in zip(pairs, want_done) if d]
    if not built:
        return r
    fbuf, fidx, rbuf, ridx = P.texts(built)
    hbuf, hidx, haux = CT.contigs_from_fastq(fbuf, fidx, rbuf, ridx, offset, prm[0], prm[1], prm[2], insert, deltaq, mode, cap, trim, threads=4)
    sel = np.nonzero(want_done)[0]
    got = P.records(r.cbuf, r.cidx[sel])
    want = P.records(hbuf, hidx)
    # the header token is the pair's own (its name carries its position in the text it came from); contig and qualities the host's
    all_f, all_fidx = texts[0].tobytes(), texts[1]
    bad = [int(i) for k, i in enumerate(sel)
           if got[k][0] != all_f[all_fidx[i, 0]:all_fidx[i, 0] + all_fidx[i, 1]] or got[k][1:] != want[k][1:]]
    assert not bad, bad[:10]
    assert np.array_equal(r.aux[sel], haux)
    assert np.array_equal(r.cidx[sel][:, 1], all_fidx[sel, 1]) and np.array_equal(r.cidx[sel][:, 3::2], hidx[:, 3::2])   # the three lengths
    assert np.array_equal(r.cidx[sel][:, 0], sel * r.rec_cap)                        # ... and where the slots lie
    assert np.array_equal(r.cidx[sel][:, 2], r.cidx[sel][:, 0] + r.cidx[sel][:, 1])
    assert np.array_equal(r.cidx[sel][:, 4], r.cidx[sel][:, 2] + r.cidx[sel][:, 3])
    for k in sel[:: max(1, len(sel) // 400)]:                                        # alignments: a spread of at most ~400 host calls
        assert alignment_of(r, k) == P.host_alignment(pairs[k], *prm), int(k)
    return r


def test_reference_alignment_fixture(eng):
    """All 4,808 alignments and scores of tests/golden/nw_pairs.npz (the reference's Cython aligner), one call per parameter
    setting; every pair is eligible, so done is all ones."""
    fx = P.fixture_alignments()
    for prm in sorted({f[1] for f in fx}):
        rows = [f for f in fx if f[1] == prm]
        _, r = device(eng, [f[0] for f in rows], prm)
        assert r.done.all() and r.n_handed_back == 0
        bad = [k for k, f in enumerate(rows) if alignment_of(r, k) != (f[2], f[3], f[4])]
        assert not bad, (prm, bad[:10])


def test_reference_contig_fixture(eng):
    """All 2,565 contigs of tests/golden/nw_contigs.npz (moira.py's make_contig): contig, qualities, overlap / gaps / mismatches."""
    rows, insert, deltaq = P.fixture_contigs()
    groups = {}
    for k, row in enumerate(rows):
        groups.setdefault(row[1:5], []).append(k)
    for (prm, mode, cap, trim), ks in groups.items():
        _, r = device(eng, [rows[k][0] for k in ks], prm, insert, deltaq, mode, cap, trim, alignments=False)
        assert r.done.all()
        recs = P.records(r.cbuf, r.cidx)
        bad = [k for n, k in enumerate(ks) if (recs[n][1].decode("latin-1"), recs[n][2], tuple(r.aux[n])) != (rows[k][5], rows[k][6], rows[k][7])]
        assert not bad, (prm, mode, cap, trim, bad[:10])


@pytest.mark.parametrize("prm", SETTINGS, ids=lambda p: "m%d_x%d_g%d" % p)
def test_length_sweep(eng, prm):
    """The whole product: (l1, l2) over the square of the C boundaries and size-class edges (361 cells) x the five sequence
    kinds, per parameter setting -- 1,805 pairs a call, 5,415 in all."""
    rng = np.random.default_rng(SETTINGS.index(prm) + 7)
    pairs = [P.make_pair(rng, l1, l2, kind) for l1 in EDGE for l2 in EDGE for kind in KINDS]
    assert len(pairs) == 19 * 19 * 5
    assert_equals_host(eng, pairs, prm)


@pytest.mark.parametrize("kind", KINDS)
def test_every_kind_at_the_column_boundaries(eng, kind):
    """Every sequence kind at every length of the sweep against itself and its neighbours (the diagonal band of the square)."""
    rng = np.random.default_rng(KINDS.index(kind) + 31)
    pairs = [P.make_pair(rng, EDGE[a], EDGE[b], kind) for a in range(len(EDGE)) for b in range(max(0, a - 1), min(len(EDGE), a + 2))]
    for prm in SETTINGS:
        assert_equals_host(eng, pairs, prm)


def mixed_batch(seed=3, n=96):
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 385, (n, 2))
    return [P.make_pair(rng, int(a), int(b), KINDS[k % 5]) for k, (a, b) in enumerate(lens)]


@pytest.mark.parametrize("setting", P.fixture_settings(), ids=lambda s: "%s_cap%d_trim%d" % s)
def test_every_consensus_cap_and_trim_setting_of_the_fixture(eng, setting):
    mode, cap, trim = setting
    assert_equals_host(eng, mixed_batch(), (1, -1, -2), 20, 6, mode, cap, trim)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_batch_sizes_and_repeatability(eng, n):
    pairs = mixed_batch(seed=n, n=n)
    a = assert_equals_host(eng, pairs, mode="posterior")
    _, b = device(eng, pairs, mode="posterior")
    assert np.array_equal(a.cidx, b.cidx) and np.array_equal(a.aux, b.aux) and np.array_equal(a.aln_len, b.aln_len) and np.array_equal(a.score, b.score)
    assert P.records(a.cbuf, a.cidx) == P.records(b.cbuf, b.cidx)


def test_empty_chunk(eng):
    r = eng.contigs_text(b"", np.zeros((0, 6), np.int64), b"", np.zeros((0, 6), np.int64))
    assert len(r.done) == 0 and r.n_done == 0 and r.n_handed_back == 0


def handback_batch():
    """Eligible pairs around one of each kind the device does not take -> (pairs, done expected per pair for sum / offset 33)."""
    rng = np.random.default_rng(77)
    good = lambda: P.make_pair(rng, int(rng.integers(20, 200)), int(rng.integers(20, 200)), "overlap")
    pairs, done = [], []
    def add(p, d):
        pairs.append(p); done.append(d)
    add(good(), True)
    add(P.make_pair(rng, 385, 100, "overlap"), False)                                # a 385-base read
    add(good(), True)
    p = good(); p.fwd = p.fwd[:40] + "a" + p.fwd[41:]                               # a lower-case base in the FORWARD read: no complement is asked of it
    add(p, True)
    p = good(); p.rev = p.rev[:7] + "c" + p.rev[8:]                                 # ... in the reverse read: no complement
    add(p, False)
    add(good(), True)
    p = good(); q = bytearray(p.fq); q[11] = 32; p.fq = bytes(q)                    # a quality below the offset
    add(p, False)
    add(good(), True)
    p = P.make_pair(rng, 90, 90, "identical", qlo=112, qhi=113)                     # sum: 112 + 112 + 33 = 257 > 255
    add(p, False)
    add(good(), True)
    add(P.Pair("ACGTACGTAC", b"IIIIIIIIII", "", b""), False)                        # an empty read: "an aligned read has no bases" on the host
    add(good(), True)
    p = good(); p.fwd = p.fwd[:-5] + "-" + p.fwd[-4:]                               # a '-' in the forward read, inside the overlap: the host
    add(p, False)                                                                    # takes it for a gap of the alignment and builds the pair
    p = good(); p.rev = p.rev[:-5] + "-" + p.rev[-4:]                               # ... in the reverse read
    add(p, False)
    add(good(), True)
    return pairs, done


def test_hand_back(eng):
    """done is 0 exactly at the pairs the device does not take; every neighbour's slot is the host's."""
    pairs, done = handback_batch()
    assert_equals_host(eng, pairs, mode="sum", cap=0, expect_done=done)
    assert done.count(False) == 7 and len(pairs) == 15
    # the same batch under parameters whose scores could leave 16 bits: every pair goes back
    _, r = device(eng, pairs, (500, -700, -900), mode="sum", cap=0)
    assert not r.done.any() and r.n_handed_back == len(pairs)


def test_contigs_from_fastq_with_an_engine_returns_or_raises_what_the_host_does(eng):
    pairs, done = handback_batch()
    for subset, kw in ((pairs[:4], dict(consensus_qscore="sum", qscore_cap=0)),                      # one hand-back the host builds (385 bases)
                       ([p for p, d in zip(pairs, done) if d], dict(consensus_qscore="posterior")),
                       (pairs[:4], dict(match=500, mismatch=-700, gap=-900))):                     # all handed back: the 32-bit path
        fbuf, fidx, rbuf, ridx = P.texts(subset)
        want = CT.contigs_from_fastq(fbuf, fidx, rbuf, ridx, 33, threads=4, **kw)
        got = CT.contigs_from_fastq(fbuf, fidx, rbuf, ridx, 33, threads=4, engine=eng, **kw)
        assert P.records(got[0], got[1]) == P.records(want[0], want[1])
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    seen = set()
    for bad_at in (4, 6, 8, 10):                                                     # no complement; negative quality; contig quality past its byte; an empty read
        subset = pairs[:3] + [pairs[bad_at]]                                         # (pair 1 is handed back too, and builds on the host)
        fbuf, fidx, rbuf, ridx = P.texts(subset)
        outcome = []
        for e in (None, eng):
            try:
                CT.contigs_from_fastq(fbuf, fidx, rbuf, ridx, 33, consensus_qscore="sum", qscore_cap=0, threads=1, engine=e)
                outcome.append(None)
            except (ValueError, CT.QualityRange) as ex:
                outcome.append((type(ex), str(ex)))
        assert outcome[0] is not None and outcome[0] == outcome[1], (bad_at, outcome)
        seen.add(outcome[0][1])
    assert len(seen) == 4 and "an aligned read has no bases" in seen                 # four different errors, each the host's own
    with pytest.raises(ValueError, match="insert must be a positive integer"):
        CT.contigs_from_fastq(*P.texts(pairs[:1]), 33, insert=0, engine=eng)


# ---- the edges of the domain: tests/golden/nw_domain.npz, the REFERENCE's answers (tests/golden/make_nw_domain.py) -------------

def assert_index_layout(r, sel, fidx, clens):
    """The index rows of the built pairs `sel`, as assert_equals_host checks them: the header's length, the contig's twice, and
    the three pieces back to back at the start of the pair's own slot."""
    rows = r.cidx[sel]
    assert np.array_equal(rows[:, 1], fidx[sel, 1]) and np.array_equal(rows[:, 3], clens) and np.array_equal(rows[:, 5], clens)
    assert np.array_equal(rows[:, 0], sel * r.rec_cap)
    assert np.array_equal(rows[:, 2], rows[:, 0] + rows[:, 1]) and np.array_equal(rows[:, 4], rows[:, 2] + rows[:, 3])


def assert_equals_reference(eng, cases):
    """One group of nw_domain.npz (one scoring and consensus setting, one offset) in one call with alignments: done is the
    fixture's `built`, and every built pair carries the reference's aligned strings, score, contig, quality bytes and overlap /
    gaps / mismatches; a second call without alignments returns the same slots and statistics."""
    prm, mode, cap, trim, insert, deltaq, offset = cases[0].group()
    pairs = [c.pair for c in cases]
    (fbuf, fidx, _, _), r = device(eng, pairs, prm, insert, deltaq, mode, cap, trim, offset)
    assert r.done.tolist() == [c.built for c in cases], (cases[0].group(), [c.k for c, d in zip(cases, r.done) if d != c.built][:10])
    sel = np.nonzero(r.done)[0]
    assert (r.n_done, r.n_handed_back) == (len(sel), len(cases) - len(sel))
    if not len(sel):
        return
    recs, text = P.records(r.cbuf, r.cidx[sel]), fbuf.tobytes()
    bad = [cases[i].k for n, i in enumerate(sel)
           if alignment_of(r, i) != (cases[i].aln1, cases[i].aln2, cases[i].score) or
           (recs[n][1].decode("latin-1"), recs[n][2], tuple(r.aux[i])) != (cases[i].contig, cases[i].cq, cases[i].stats) or
           recs[n][0] != text[fidx[i, 0]:fidx[i, 0] + fidx[i, 1]]]
    assert not bad, (cases[0].group(), bad[:10])
    assert_index_layout(r, sel, fidx, np.array([len(cases[i].contig) for i in sel]))
    _, q = device(eng, pairs, prm, insert, deltaq, mode, cap, trim, offset, alignments=False)
    assert np.array_equal(q.done, r.done) and np.array_equal(q.cidx[sel], r.cidx[sel]) and np.array_equal(q.aux[sel], r.aux[sel])
    assert P.records(q.cbuf, q.cidx[sel]) == recs and q.rec_cap == r.rec_cap


DOMAIN_SLICES = {"alignments": lambda c: c.part <= 2, "contigs_offset_33": lambda c: c.part >= 3 and c.offset == 33,
                 "contigs_offset_64": lambda c: c.part >= 3 and c.offset == 64, "contigs_offset_0": lambda c: c.part >= 3 and c.offset == 0}


@pytest.mark.parametrize("which", list(DOMAIN_SLICES))
def test_reference_domain_fixture(eng, which):
    """The whole of nw_domain.npz, one call per (scoring, consensus, cap, trim, insert, deltaq, offset) group: scoring sets up to
    the 16-bit predicate (scores near +-30,000 in the fix-up's packed keys), zero / negative / sign-reversed parameters, every
    outcome of the 3' fix-up, fifteen IUPAC letters, offsets 0 / 33 / 64, qualities 0..128 (the posterior tables far outside their
    40 x 40 corner), contig qualities that leave their byte or fall below zero (handed back)."""
    groups = {}
    for c in P.fixture_domain():
        if DOMAIN_SLICES[which](c):
            groups.setdefault(c.group(), []).append(c)
    assert len(groups) >= 19 and sum(len(g) for g in groups.values()) >= 250
    for cases in groups.values():
        assert_equals_reference(eng, cases)


def test_predicate_boundary(eng):
    """(l1 + l2 + 2) * max|param| against 30,000, four values of max|param|: the fixture's pair just below (29,900..29,999; built,
    the reference's alignment) and the one at or just above (30,000..30,100; handed back) between ordinary pairs in one call,
    whose slots are the host's."""
    rows = [c for c in P.fixture_domain() if c.part == 1]
    assert len(rows) == 8
    rng = np.random.default_rng(30000)
    for below, above in zip(rows[0::2], rows[1::2]):
        prm, m = below.prm, max(abs(v) for v in below.prm)
        assert above.prm == prm and below.built and not above.built
        assert 29900 <= (len(below.pair.fwd) + len(below.pair.rev) + 2) * m <= 29999
        assert 30000 <= (len(above.pair.fwd) + len(above.pair.rev) + 2) * m <= 30100
        plain = lambda: P.make_pair(rng, int(rng.integers(20, 60)), int(rng.integers(20, 60)), "overlap")
        pairs = [plain(), below.pair, plain(), above.pair, plain()]
        r = assert_equals_host(eng, pairs, prm, expect_done=[True, True, True, False, True])
        assert alignment_of(r, 1) == (below.aln1, below.aln2, below.score)
        assert (P.records(r.cbuf, r.cidx[1:2])[0][1:], tuple(r.aux[1])) == ((below.contig.encode("latin-1"), below.cq), below.stats)


def lds_size_classes(tmp_path):
    """(the class caps of mpb_contig.cpp, cd_lds_bytes as an int32[384, 384] of (l1 - 1, l2 - 1)): the caps from the source's
    own table, the sizes from the model checker's --lds mode, so that nothing of the layout is restated here."""
    import re
    import subprocess
    from test_contig_device_model import build_checker
    exe, out = build_checker(str(tmp_path / "check")), str(tmp_path / "lds.bin")
    subprocess.check_call([exe, "--lds", out])
    raw = np.fromfile(out, np.int32)
    lds_max, max_len = int(raw[0]), int(raw[1])
    src = open(os.path.join(ROOT, "moira_amd", "csrc", "mpb_contig.cpp")).read()
    caps = [lds_max if t.strip() == "MPB_CONTIG_LDS_MAX" else int(t) for t in re.search(r"k_lds_class\[\] = \{([^}]*)\}", src).group(1).split(",")]
    return caps, raw[2:].reshape(max_len, max_len)


def test_lds_size_class_boundaries(eng, tmp_path):
    """The ten LDS size classes (one launch each): for every cap the pair with the largest cd_lds_bytes not above it and the one
    with the smallest above it -- the last pair of one launch and the first of the next -- in one call, in shuffled order,
    each between a C = 1 pair and a C = 6 pair on either side.  Every pair is built and is the host's."""
    caps, size = lds_size_classes(tmp_path)
    assert len(caps) == 10 and caps == sorted(caps) and size.max() <= caps[-1] and size.min() <= caps[0]
    edge = []
    for cap in caps:
        fits = np.where(size <= cap, size, -1)
        edge.append(np.unravel_index(int(fits.argmax()), size.shape))
        if (size > cap).any():
            edge.append(np.unravel_index(int(np.where(size > cap, size, 1 << 30).argmin()), size.shape))
    assert len(edge) == 19                               # no pair of 384 bases or fewer lies above the last cap
    rng = np.random.default_rng(4096)
    pairs = []
    for n in rng.permutation(len(edge)):
        l1, l2 = int(edge[n][0]) + 1, int(edge[n][1]) + 1
        small = lambda: P.make_pair(rng, int(rng.integers(1, 385)), int(rng.integers(1, 65)), KINDS[int(rng.integers(0, 5))])
        large = lambda: P.make_pair(rng, int(rng.integers(1, 385)), int(rng.integers(321, 385)), KINDS[int(rng.integers(0, 5))])
        pairs += [small(), large(), P.make_pair(rng, l1, l2, KINDS[n % 5]), large(), small()]
    classes = {int(np.searchsorted(caps, size[len(p.fwd) - 1, len(p.rev) - 1])) for p in pairs}
    assert classes == set(range(10))
    assert_equals_host(eng, pairs, mode="posterior")


LETTERS = "ACGTNWSRYMKBVDH"


def test_bytes_of_the_reads(eng):
    """One call: a '-' in the forward read and one in the reverse read (handed back: make_contig reads a '-' as a gap of the
    alignment, only the host reproduces that), a '.' in either read (it has a complement and aligns as a letter of its own: built,
    as the host library builds it -- the reference itself refuses a '.' in a read that has qualities, its reverse_complement
    raises LengthMismatchError; nothing is changed here), and each of the fifteen letters as the first and the last base of both
    reads (the complement of the reverse read's two ends: R <-> Y, M <-> K, B <-> V, D <-> H)."""
    rng = np.random.default_rng(15)
    good = lambda: P.make_pair(rng, int(rng.integers(30, 200)), int(rng.integers(30, 200)), "overlap")
    put = lambda s, at, ch: s[:at] + ch + s[at + 1:]
    pairs, done = [], []
    def add(p, d):
        pairs.append(p); done.append(d)
    add(good(), True)
    p = good(); p.fwd = put(p.fwd, len(p.fwd) - 6, "-"); add(p, False)
    add(good(), True)
    p = good(); p.rev = put(p.rev, len(p.rev) - 6, "-"); add(p, False)
    p = good(); p.fwd = put(p.fwd, len(p.fwd) - 6, "."); add(p, True)
    p = good(); p.rev = put(p.rev, len(p.rev) - 6, "."); add(p, True)
    p = good(); p.fwd = put(put(p.fwd, 0, "."), len(p.fwd) - 1, "."); p.rev = put(put(p.rev, 0, "."), len(p.rev) - 1, "."); add(p, True)
    for ch in LETTERS:
        p = good()
        p.fwd, p.rev = put(put(p.fwd, 0, ch), len(p.fwd) - 1, ch), put(put(p.rev, 0, ch), len(p.rev) - 1, ch)
        add(p, True)
    add(good(), True)
    for mode in ("best", "posterior"):
        r = assert_equals_host(eng, pairs, mode=mode, expect_done=done)
    recs = P.records(r.cbuf, r.cidx)
    for n, ch in enumerate(LETTERS):                     # the contig begins with the forward read's first base and ends with the
        contig = recs[7 + n][1].decode("latin-1")        # complement of the reverse record's first
        assert contig[0] == ch and contig[-1] == P.COMP[ch], (ch, contig)


# ---- the CLI ---------------------------------------------------------------------------------------------------------------------

def counting_backend():
    be = cli.make_gpu_backend(None)
    calls = []
    inner = be.engine.contigs_text

    def contigs_text(*a, **kw):
        r = inner(*a, **kw)
        calls.append((len(r.done), int(r.n_done)))
        return r
    be.engine.contigs_text = contigs_text
    return be, calls


@pytest.mark.parametrize("pack", [False, True], ids=["alone", "with_device_pack"])
def test_cli_paired_golden_command_with_device_contigs(tmp_path, pack):
    from test_cli_golden import reference_args, same_files
    out = str(tmp_path / "on")
    a = reference_args(paired=True, forward_fastq=os.path.join(GOLD, "test1.fastq.gz"), output_prefix=out,
                       reverse_fastq=os.path.join(GOLD, "test2.fastq.bz2"))
    a.device_contigs, a.device_pack = True, pack
    be, calls = counting_backend()
    try:
        assert cli.main(a, backend=be, out=open(os.devnull, "w")) == 0
    finally:
        be.engine.close()
    assert len(calls) >= 1 and sum(c[0] for c in calls) == 1000 and sum(c[1] for c in calls) == 1000   # the device built every pair
    same_files(out, "paired")                                                        # tests/golden/reference_test_results/paired.qc.*


def test_cli_with_several_chunks_makes_every_device_call_on_the_consumer_thread(tmp_path, monkeypatch):
    """Chunks of 192 pairs: six chunks of the golden input, so that reading chunk k + 1 on the producer thread runs beside the
    filter of chunk k.  Calls on one context must not overlap (include/moira_pb.h), so every call the run makes on the engine --
    the device contigs and the filter alike -- has to come from one thread, the one that runs cli.main; the files are the
    reference's."""
    import threading
    from test_cli_golden import reference_args, same_files
    monkeypatch.setattr(cli, "PAIR_CHUNK_READS", 192)
    out = str(tmp_path / "chunks")
    a = reference_args(paired=True, forward_fastq=os.path.join(GOLD, "test1.fastq.gz"), output_prefix=out,
                       reverse_fastq=os.path.join(GOLD, "test2.fastq.bz2"))
    a.device_contigs = True
    be, calls = counting_backend()
    threads = {"contigs": set(), "filter": set()}
    inner_contigs, inner_matrix = be.engine.contigs_text, be.matrix

    def contigs_text(*x, **kw):
        threads["contigs"].add(threading.get_ident())
        return inner_contigs(*x, **kw)

    def matrix(*x, **kw):
        threads["filter"].add(threading.get_ident())
        return inner_matrix(*x, **kw)
    be.engine.contigs_text, be.matrix = contigs_text, matrix
    try:
        assert cli.main(a, backend=be, out=open(os.devnull, "w")) == 0
    finally:
        be.engine.close()
    assert [c[0] for c in calls] == [192] * 5 + [40] and sum(c[1] for c in calls) == 1000
    assert threads["contigs"] == threads["filter"] == {threading.get_ident()}
    same_files(out, "paired")


def test_cli_forward_only_command_ignores_device_contigs(tmp_path):
    import io
    from test_cli_golden import reference_args, same_files
    out, msg = str(tmp_path / "fwd"), io.StringIO()
    a = reference_args(paired=False, forward_fastq=os.path.join(GOLD, "test1.fastq.gz"), output_prefix=out)
    a.device_contigs = True
    be, calls = counting_backend()
    try:
        assert cli.main(a, backend=be, out=msg) == 0
    finally:
        be.engine.close()
    assert calls == [] and len([l for l in msg.getvalue().split("\n") if "--device_contigs does not apply" in l]) == 1
    same_files(out, "forward")
