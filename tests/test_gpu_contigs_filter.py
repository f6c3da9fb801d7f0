"""The fused contig-and-filter call on the GPU (include/moira_pb.h: mpb_contigs_filter_text_host, k_contig_rows;
Engine.contigs_filter_text, moira_amd.contig.contigs_from_fastq_filtered, the CLI with --device_contigs --device_pack).  The
reference everywhere is the two-call sequence it joins, on the same engine: contigs_text, then filter_text(cbuf, cidx, sel = the
pairs the device built); everything is compared bit for bit (ee as uint64), with the default exact arithmetic.  The per-pair
code of k_contig_rows on the host, with damaged index rows: tests/test_contig_rows_model.py; the merge of handed-back pairs
without a device: tests/test_contigs_filter_merge.py."""
import os
import threading

import numpy as np
import pytest

from helpers import contig_pairs as P
from moira_amd import cli
from moira_amd import contig as CT
from moira_amd import engine as E

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
RESULTS = ("ee", "ns", "passed", "lens", "has_n")


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(0)
    yield e
    e.close()


def assert_eligible(pairs, offset=33, prm=(1, -1, -2)):
    """The header's conditions for a pair the device takes, restated on the CPU (the contig qualities: by the caller's choice of
    qualities and mode): lengths 1..384, the 16-bit predicate, bases with a complement and no '-', no quality below the offset."""
    for p in pairs:
        assert 1 <= len(p.fwd) <= 384 and 1 <= len(p.rev) <= 384
        assert (len(p.fwd) + len(p.rev) + 2) * max(abs(v) for v in prm) < 30000
        assert set(p.rev) <= set("ACGTN") and "-" not in p.fwd and min(p.fq + p.rq) >= offset


def at_offset(p, offset):
    """The pair with its quality lines moved from offset 33 to `offset`."""
    return P.Pair(p.fwd, bytes(b - 33 + offset for b in p.fq), p.rev, bytes(b - 33 + offset for b in p.rq))


def two_calls(eng, texts, offset, ckw, fkw):
    r = eng.contigs_text(*texts, offset, **ckw)
    sel = np.nonzero(r.done)[0]
    f = eng.filter_text(r.cbuf, r.cidx, sel=sel, fastq_offset=offset, **fkw)
    return r, sel, f


def assert_fused_equals_two_calls(eng, pairs, offset=33, ckw=None, fkw=None, all_built=True, ref=None):
    ckw, fkw = ckw or {}, fkw or {}
    texts = P.texts(pairs)
    r, sel, f = ref or two_calls(eng, texts, offset, ckw, fkw)
    g = eng.contigs_filter_text(*texts, offset, **ckw, **fkw)
    assert g.filter_error is None
    assert np.array_equal(g.done, r.done) and np.array_equal(g.filtered, g.done)
    assert (g.n_done, g.n_handed_back) == (r.n_done, r.n_handed_back)
    if all_built:
        assert g.n_handed_back == 0 and g.filtered.all()
    for name in RESULTS:
        a, b = getattr(g, name)[sel], getattr(f, name)
        if name == "ee":
            a, b = a.view(np.uint64), np.ascontiguousarray(b).view(np.uint64)
        assert np.array_equal(a, b), (name, np.nonzero(a != b)[0][:10])
    assert (g.n_pass, g.n_overflow) == (f.n_pass, f.n_overflow)
    assert np.array_equal(g.cidx[sel], r.cidx[sel]) and np.array_equal(g.aux[sel], r.aux[sel]) and g.rec_cap == r.rec_cap
    assert P.records(g.cbuf, g.cidx[sel]) == P.records(r.cbuf, r.cidx[sel])
    return g, (r, sel, f)


def test_lengths(eng):
    """(l1, l2) over the square of the column boundaries, the overlap and unrelated kinds, in one call: 338 pairs, all built."""
    edge = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 383, 384)
    rng = np.random.default_rng(1)
    pairs = [P.make_pair(rng, a, b, kind) for a in edge for b in edge for kind in ("overlap", "unrelated")]
    assert len(pairs) == 338
    assert_eligible(pairs)
    g, _ = assert_fused_equals_two_calls(eng, pairs)
    assert g.lens.min() >= 1 and g.lens.max() >= 384 and g.lens.tolist() == g.cidx[:, 5].tolist()


def test_hand_back_interleaved(eng):
    """The mixed batch of tests/test_gpu_contigs.py (reads of 0 and 385 bases, a base without a complement, a quality below the
    offset, a contig quality past its byte, a '-' in either read, among eligible pairs): filtered == done, values equal on the
    built pairs; and through contigs_from_fastq_filtered every pair -- of the sub-batch the host can build at all -- is the
    all-host path's."""
    from test_gpu_contigs import handback_batch
    pairs, done = handback_batch()
    ckw = dict(consensus=P.MODES["sum"], qscore_cap=0)
    g, _ = assert_fused_equals_two_calls(eng, pairs, ckw=ckw, all_built=False)
    assert g.done.tolist() == done and g.n_handed_back == 7
    buildable = [p for k, p in enumerate(pairs) if k not in (4, 6, 8, 10)]           # (the four the host raises for)
    texts = P.texts(buildable)
    hbuf, hidx, haux = CT.contigs_from_fastq(*texts, 33, consensus_qscore="sum", qscore_cap=0, threads=4)
    want = eng.filter_text(hbuf, hidx)
    cbuf, cidx, aux, ee, has_n, err = CT.contigs_from_fastq_filtered(*texts, 33, consensus_qscore="sum", qscore_cap=0, threads=4, engine=eng)
    assert err is None
    assert np.array_equal(cidx, hidx) and np.array_equal(aux, haux) and P.records(cbuf, cidx) == P.records(hbuf, hidx)
    assert np.array_equal(ee.view(np.uint64), want.ee.view(np.uint64)) and np.array_equal(has_n, want.has_n)


@pytest.fixture(scope="module")
def pairs_150():
    rng = np.random.default_rng(150)
    pairs = [P.make_pair(rng, 150, 150, ("overlap", "unrelated", "contained")[k % 3]) for k in range(100)]
    assert_eligible(pairs)
    return pairs


@pytest.mark.parametrize("max_len", (1, 100, 128, 129, 600))
def test_truncation(eng, pairs_150, max_len):
    g, _ = assert_fused_equals_two_calls(eng, pairs_150, fkw=dict(max_len=max_len))
    assert g.lens.tolist() == np.minimum(g.cidx[:, 5], max_len).tolist() and 150 <= g.cidx[:, 5].max() <= 300


def with_ambiguous_bases(pairs):
    """'N' and 'n' in the part of the forward read the mate does not reach, an 'N' in the part of the mate past the forward read
    (the head of the reverse record): none of them is asked for a complement it does not have."""
    out = []
    for k, p in enumerate(pairs):
        f, r = list(p.fwd), list(p.rev)
        if k % 2 == 0:
            f[1] = "N"
        if k % 3 == 0:
            f[3] = "n"
        if k % 5 == 0:
            r[0] = "N"
        out.append(P.Pair("".join(f), p.fq, "".join(r), p.rq))
    return out


BYTE_CASES = {
    "N_lower_is_ambiguous": dict(ambiguous=True, fkw=dict(lower_n_is_base=False)),
    "N_lower_is_base": dict(ambiguous=True, fkw=dict(lower_n_is_base=True)),
    "N_disallowed": dict(ambiguous=True, fkw=dict(ambigs="disallow")),
    "offset_64": dict(offset=64),
    "offset_0": dict(offset=0),
    "best_cap0": dict(ckw=dict(consensus=0, qscore_cap=0)),
    "sum": dict(ckw=dict(consensus=1)),
    "posterior": dict(ckw=dict(consensus=2)),
    "trim_overlap": dict(ckw=dict(trim_overlap=True)),
    "sum_trim_offset_64": dict(offset=64, ckw=dict(consensus=1, trim_overlap=True)),
}


@pytest.mark.parametrize("case", list(BYTE_CASES))
def test_bytes(eng, case):
    c = BYTE_CASES[case]
    rng = np.random.default_rng(len(case))
    pairs = [P.make_pair(rng, 150, 140, "overlap") for _ in range(60)]
    if c.get("ambiguous"):
        pairs = with_ambiguous_bases(pairs)
    offset = c.get("offset", 33)
    pairs = [at_offset(p, offset) for p in pairs]
    assert_eligible(pairs, offset)
    g, _ = assert_fused_equals_two_calls(eng, pairs, offset, c.get("ckw"), c.get("fkw"))
    if c.get("ambiguous"):
        assert g.has_n.sum() >= 30 and g.ns.max() >= 1


def test_piece_loop(eng, monkeypatch):
    """Pieces of two rows (the bound of 2 x 150 is a 384-byte row): 25 trips through pack, status and filter."""
    rng = np.random.default_rng(50)
    pairs = [P.make_pair(rng, 150, 150, "overlap") for _ in range(50)]
    assert_eligible(pairs)
    texts = P.texts(pairs)
    ref = two_calls(eng, texts, 33, {}, {})
    monkeypatch.setenv("MPB_TEXT_PIECE_BYTES", str(2 * 384))
    assert_fused_equals_two_calls(eng, pairs, ref=ref)


@pytest.mark.parametrize("device_tail", [False, True], ids=["host_tail", "device_tail"])
def test_poisson(eng, pairs_150, device_tail):
    fkw = dict(poisson=True, poisson_device_tail=True) if device_tail else dict(poisson=True)
    assert_fused_equals_two_calls(eng, pairs_150, fkw=fkw)


def test_filter_refusal(eng):
    """A chunk with one contig quality of 255 at offset 0 (mode sum, no cap: 127 + 128 where the two reads agree -- found with the
    host library first): the byte packs to Q255, which k_pack_text reports.  The contigs are complete and equal, nothing counts
    as filtered, and filter_error is what filter_text raises over the built pairs -- the bad pair's position among THEM (a
    handed-back pair lies before it)."""
    rng = np.random.default_rng(255)
    good = lambda: at_offset(P.make_pair(rng, 100, 100, "overlap"), 0)
    hot = P.make_pair(rng, 90, 90, "identical")
    hot = P.Pair(hot.fwd, bytes([127]) * 90, hot.rev, bytes([128]) * 90)
    long_one = at_offset(P.make_pair(rng, 385, 50, "overlap"), 0)                    # handed back
    pairs = [good(), long_one, good(), good(), hot, good()]
    ckw = dict(consensus=P.MODES["sum"], qscore_cap=0)
    _, _, _, _, hbuf, hidx, _ = P.host_contigs(pairs, offset=0, consensus="sum", cap=0)
    assert 255 in P.records(hbuf, hidx)[4][2] and all(255 not in rec[2] for k, rec in enumerate(P.records(hbuf, hidx)) if k != 4)
    texts = P.texts(pairs)
    r = eng.contigs_text(*texts, 0, **ckw)
    sel = np.nonzero(r.done)[0]
    assert sel.tolist() == [0, 2, 3, 4, 5]
    with pytest.raises(ValueError) as want:
        eng.filter_text(r.cbuf, r.cidx, sel=sel, fastq_offset=0)
    assert want.value.bad_record == 3 and "254" in str(want.value)
    g = eng.contigs_filter_text(*texts, 0, **ckw)
    assert np.array_equal(g.done, r.done) and not g.filtered.any() and g.n_pass == 0
    assert np.array_equal(g.cidx[sel], r.cidx[sel]) and np.array_equal(g.aux[sel], r.aux[sel])
    assert P.records(g.cbuf, g.cidx[sel]) == P.records(r.cbuf, r.cidx[sel])
    assert isinstance(g.filter_error, ValueError) and str(g.filter_error) == str(want.value) and g.filter_error.bad_record == 3
    # ... and the same engine filters the next chunk
    assert_fused_equals_two_calls(eng, [good() for _ in range(5)], 0, ckw)


@pytest.mark.parametrize("offset", [33, 64, 0])
def test_reference_domain_fixture(eng, offset):
    """The contig cases of tests/golden/nw_domain.npz (qualities 0..128, every consensus setting, exotic scoring, hand-backs in
    between) at one offset, one fused call per (scoring, consensus, cap, trim, insert, deltaq) group against the two calls it
    joins: done, slots, ee, ns, pass and the counts are equal; where filter_text refuses the built contigs for a quality out of
    range, the fused call reports the same error for the same record and counts nothing as filtered."""
    groups = {}
    for c in P.fixture_domain():
        if c.part >= 3 and c.offset == offset:
            groups.setdefault(c.group(), []).append(c)
    assert len(groups) >= 50 and sum(len(g) for g in groups.values()) >= 250
    refused = 0
    for (prm, mode, cap, trim, insert, deltaq, _), cases in groups.items():
        ckw = dict(match=prm[0], mismatch=prm[1], gap=prm[2], insert=insert, deltaq=deltaq, consensus=P.MODES[mode], qscore_cap=cap,
                   trim_overlap=trim)
        texts = P.texts([c.pair for c in cases])
        r = eng.contigs_text(*texts, offset, **ckw)
        assert r.done.tolist() == [c.built for c in cases]
        sel = np.nonzero(r.done)[0]
        try:
            f = eng.filter_text(r.cbuf, r.cidx, sel=sel, fastq_offset=offset)
        except ValueError as want:
            g = eng.contigs_filter_text(*texts, offset, **ckw)
            assert np.array_equal(g.done, r.done) and not g.filtered.any() and g.n_pass == 0
            assert isinstance(g.filter_error, ValueError) and str(g.filter_error) == str(want)
            assert g.filter_error.bad_record == want.bad_record and 0 <= want.bad_record < len(sel)
            assert P.records(g.cbuf, g.cidx[sel]) == P.records(r.cbuf, r.cidx[sel])
            refused += 1
            continue
        assert_fused_equals_two_calls(eng, [c.pair for c in cases], offset, ckw, all_built=False, ref=(r, sel, f))
    assert (refused >= 1) == (offset == 0)               # the fixture's two contigs with the byte 255 (127 + 128 at offset 0)


def test_reuse(eng):
    """Three calls of different sizes on one engine (the staging blocks grow once and are then reused by smaller chunks), each
    equal to its own reference; a plain filter() before and after gives identical results."""
    rng = np.random.default_rng(8)
    q = rng.integers(2, 42, (500, 128)).astype(np.uint8)
    lens = rng.integers(1, 129, 500).astype(np.int32)
    for i in range(500):
        q[i, lens[i]:] = 0
    before = eng.filter(q, lens=lens)
    for n in (300, 7, 120):
        pairs = [P.make_pair(rng, int(rng.integers(20, 300)), int(rng.integers(20, 300)), "overlap") for _ in range(n)]
        assert_eligible(pairs)
        assert_fused_equals_two_calls(eng, pairs)
    after = eng.filter(q, lens=lens)
    assert np.array_equal(before.ee.view(np.uint64), after.ee.view(np.uint64)) and np.array_equal(before.ns, after.ns)
    assert np.array_equal(before.passed, after.passed) and (before.n_pass, before.n_overflow) == (after.n_pass, after.n_overflow)


def test_kernel_times_name_the_two_contig_kernels(eng, pairs_150):
    eng.timing(True)
    try:
        eng.timing_reset()
        eng.contigs_filter_text(*P.texts(pairs_150), 33)
        t = eng.kernel_times()
    finally:
        eng.timing(False)
    assert t["contig"][1] >= 1 and t["contig_rows"][1] == 1 and t["pack_text"][1] == 1 and t["contig"][0] > 0


# ---- the CLI ---------------------------------------------------------------------------------------------------------------------

def spying_backend():
    be = cli.make_gpu_backend(None)
    seen = {"fused": [], "filter_text": [], "threads": set()}
    inner_fused, inner_text = be.engine.contigs_filter_text, be.engine.filter_text

    def contigs_filter_text(*a, **kw):
        seen["threads"].add(threading.get_ident())
        r = inner_fused(*a, **kw)
        seen["fused"].append((len(r.done), np.nonzero(~r.filtered)[0].tolist(), r.filter_error))
        return r

    def filter_text(buf, idx, sel=None, **kw):
        seen["threads"].add(threading.get_ident())
        seen["filter_text"].append(None if sel is None else np.asarray(sel).tolist())
        return inner_text(buf, idx, sel=sel, **kw)
    be.engine.contigs_filter_text, be.engine.filter_text = contigs_filter_text, filter_text
    return be, seen


def run_cli(tmp_path, name, device_contigs, device_pack):
    from test_cli_golden import reference_args, same_files
    out = str(tmp_path / name)
    a = reference_args(paired=True, forward_fastq=os.path.join(GOLD, "test1.fastq.gz"), output_prefix=out,
                       reverse_fastq=os.path.join(GOLD, "test2.fastq.bz2"))
    a.device_contigs, a.device_pack = device_contigs, device_pack
    be, seen = spying_backend()
    try:
        assert cli.main(a, backend=be, out=open(os.devnull, "w")) == 0
    finally:
        be.engine.close()
    same_files(out, "paired")                                                        # tests/golden/reference_test_results/paired.*
    return seen


def test_cli_with_both_switches_makes_one_fused_call_per_chunk(tmp_path, monkeypatch):
    """Chunks of 192 pairs, six of the golden input: one fused call each, all from the thread that runs cli.main, no filter_text
    call but for the pairs a fused call left unfiltered; the files are the reference's byte for byte."""
    monkeypatch.setattr(cli, "PAIR_CHUNK_READS", 192)
    seen = run_cli(tmp_path, "both", True, True)
    assert [c[0] for c in seen["fused"]] == [192] * 5 + [40] and all(c[2] is None for c in seen["fused"])
    assert seen["filter_text"] == [c[1] for c in seen["fused"] if c[1]]
    assert seen["threads"] == {threading.get_ident()}


@pytest.mark.parametrize("which", ["device_contigs", "device_pack"])
def test_cli_with_either_switch_alone_never_makes_the_fused_call(tmp_path, monkeypatch, which):
    monkeypatch.setattr(cli, "PAIR_CHUNK_READS", 192)
    seen = run_cli(tmp_path, which, which == "device_contigs", which == "device_pack")
    assert seen["fused"] == []
    assert (len(seen["filter_text"]) == 6 and all(s is None for s in seen["filter_text"])) if which == "device_pack" else seen["filter_text"] == []
