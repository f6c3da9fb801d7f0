"""Paired FASTQ from text alone on the GPU (include/moira_pb.h: mpb_contigs_filter_fastq_host; Engine.contigs_filter_fastq; the
CLI's --device_pair_index).  Every case compares the text-alone call with what the host builds today -- fastio.index x 2,
fastio.first_header_mismatch and Engine.contigs_filter_text on the two indexes cut to the built pairs (helpers.pair_index_inputs.
reference) -- bit for bit on every output; that path is pinned to the reference by tests/test_gpu_contigs.py and
tests/test_gpu_contigs_filter.py.  The per-lane code of the pairing kernels on the host: tests/test_pair_lane_model.py."""
import gzip
import io
import os
import threading

import numpy as np
import pytest

from helpers import contig_pairs as P
from helpers import pair_index_inputs as X
from moira_amd import _lib as L
from moira_amd import cli
from moira_amd import engine as E
from moira_amd import fastio

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
RES = os.path.join(GOLD, "reference_test_results")


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(0)
    yield e
    e.close()


def check(eng, ftext, rtext, **kw):
    idx_kw = {k: kw.pop(k) for k in ("idx_cap_rows", "out_cap_bytes") if k in kw}
    want = X.reference(eng, ftext, rtext, **kw)
    got = eng.contigs_filter_fastq(ftext, rtext, **kw, **idx_kw)
    X.assert_same(got, want)
    return got


def some_pairs(n, seed=5, lo=20, hi=120):
    rng = np.random.default_rng(seed)
    return [P.make_pair(rng, int(rng.integers(lo, hi)), int(rng.integers(lo, hi)), "overlap") for _ in range(n)]


@pytest.mark.parametrize("n", (1, 63, 64, 65, 255, 256, 257))
def test_pair_counts_across_wave_and_workgroup_borders(eng, n):
    """The ranks of k_pair_lists across the borders of a wave (64) and a workgroup (256): lengths of three size classes mixed."""
    rng = np.random.default_rng(n)
    pairs = [P.make_pair(rng, (30, 150, 250)[int(rng.integers(0, 3))], (40, 140, 251)[int(rng.integers(0, 3))], "overlap") for _ in range(n)]
    got = check(eng, *X.pair_texts(pairs))
    assert got.n_built == n and got.n_handed_back == 0


def test_all_ten_classes_with_hand_backs_interleaved(eng):
    """600 pairs of 1..384 bases over all ten size classes (tests/test_pair_lane_model.py checks on the host that the lengths
    reach every class and that the host model takes every one), with pairs that must be handed back in between: a 385-base read,
    a base without a complement, a '-' in a read.  Exactly those are handed back."""
    pairs = X.class_pairs()
    rng = np.random.default_rng(2)
    back = 0
    for k in range(7, len(pairs), 23):
        kind = (k // 23) % 3
        if kind == 0:
            pairs[k] = P.make_pair(rng, 385, 100, "unrelated")
        elif kind == 1:
            p = pairs[k] = P.make_pair(rng, 90, 80, "overlap")
            p.rev = p.rev[:40] + "X" + p.rev[41:]
        else:
            p = pairs[k] = P.make_pair(rng, 70, 95, "overlap")
            p.fwd = p.fwd[:10] + "-" + p.fwd[11:]
        back += 1
    got = check(eng, *X.pair_texts(pairs))
    assert got.n_built == 600 and got.n_handed_back == back and got.n_done == 600 - back


@pytest.mark.parametrize("consensus,trim,max_len,poisson,offset",
                         [(0, False, 0, False, 33), (1, True, 0, False, 33), (2, False, 100, False, 33), (0, True, 100, True, 33),
                          (2, True, 0, True, 64), (1, False, 0, False, 64)])
def test_settings(eng, consensus, trim, max_len, poisson, offset):
    pairs = some_pairs(130, seed=consensus + 3 * offset, lo=1, hi=300)
    if offset != 33:
        for p in pairs:
            p.fq = bytes(b + offset - 33 for b in p.fq)
            p.rq = bytes(b + offset - 33 for b in p.rq)
    check(eng, *X.pair_texts(pairs), fastq_offset=offset, consensus=consensus, trim_overlap=trim, max_len=max_len, poisson=poisson)


@pytest.mark.parametrize("at", (0, 150, 299))
@pytest.mark.parametrize("how", ("length", "last_byte"))
def test_header_mismatch(eng, at, how):
    pairs = some_pairs(300)
    names = [("read_%05d" % i).encode() for i in range(300)]
    rnames = list(names)
    rnames[at] = names[at] + b"x" if how == "length" else names[at][:-1] + b"#"
    got = check(eng, *X.pair_texts(pairs, names, rnames))
    assert (got.mismatch, got.n_built, got.n_pairs) == (at, at, 300)


@pytest.mark.parametrize("which", (0, 1))
@pytest.mark.parametrize("kind", (1, 2, 3))
def test_bad_record_in_either_file(eng, which, kind):
    pairs = some_pairs(100)
    recs = [[(("p%d" % i).encode(), p.fwd.encode(), p.fq) for i, p in enumerate(pairs)],
            [(("p%d" % i).encode(), p.rev.encode(), p.rq) for i, p in enumerate(pairs)]]
    name, seq, qual = recs[which][70]
    recs[which][70] = (name, b"" if kind == 1 else seq, b"" if kind == 2 else qual[:-1] if kind == 3 else qual)
    got = check(eng, X.fastq_text(recs[0]), X.fastq_text(recs[1]))
    bad = (got.f_bad, got.r_bad)[which]
    assert got.n_pairs == 70 and bad is not None and bad.kind == kind and (got.f_bad, got.r_bad)[1 - which] is None


def test_unequal_record_counts(eng):
    pairs = some_pairs(90)
    f, _ = X.pair_texts(pairs)
    _, r = X.pair_texts(pairs[:85])
    assert check(eng, f, r).n_pairs == 85
    assert check(eng, r, f).n_pairs == 85


def test_non_final_text_with_a_partial_record_in_one_file(eng):
    pairs = some_pairs(40)
    f, r = X.pair_texts(pairs)
    cut = f[: len(f) - 30]                                   # the last forward record is incomplete
    got = check(eng, cut, r, ffinal=False, rfinal=True)
    assert got.n_pairs == 39 and len(got.ridx) == 40 and got.f_consumed < len(cut)
    check(eng, cut, r, ffinal=False, rfinal=False)
    check(eng, r, cut, ffinal=True, rfinal=False)


def test_max_records_below_both_counts(eng):
    f, r = X.pair_texts(some_pairs(120))
    got = check(eng, f, r, max_records=50)
    assert got.n_pairs == 50 and got.f_consumed < len(f)
    assert check(eng, f, r, max_records=0).n_pairs == 0


def test_non_ascii_in_the_reverse_text_only(eng):
    f, r = X.pair_texts(some_pairs(20))
    with pytest.raises(E.NotTaken) as e:
        eng.contigs_filter_fastq(f, r[:100] + b"\x80" + r[101:])
    assert (e.value.why, e.value.which) == (L.FQ_WHY.index(str(e.value)), 1) and e.value.why == 1
    with pytest.raises(E.NotTaken) as e:
        eng.contigs_filter_fastq(f[:50] + b"\xff" + f[51:], r)
    assert (e.value.why, e.value.which) == (1, 0)


def test_both_capacities_are_asked_for_again(eng):
    f, r = X.pair_texts(some_pairs(200))
    got = check(eng, f, r, idx_cap_rows=10, out_cap_bytes=64)
    assert got.calls == 3 and got.n_built == 200
    assert check(eng, f, r, idx_cap_rows=201).calls == 1
    assert check(eng, f, r, idx_cap_rows=200).calls == 2


def test_golden_pairs(eng):
    f, r = X.golden_texts()
    got = check(eng, f, r)
    assert got.n_built == 1000 and got.mismatch == -1
    eng.timing(True)
    eng.timing_reset()
    eng.contigs_filter_fastq(f, r)
    t = eng.kernel_times()
    eng.timing(False)
    assert t["contig_rows"][0] > 0 and t["contig_rows"][1] >= 4 and t["contig"][1] >= 1
    ms, cnt = L.C.c_double(), L.C.c_int64()
    assert eng.lib.mpb_kernel_time(eng.ctx, 22, L.C.byref(ms), L.C.byref(cnt)) != 0      # no kernel id above 21 exists


# ---- the CLI ---------------------------------------------------------------------------------------------------------------------

def spying_backend():
    be = cli.make_gpu_backend(None)
    seen = {"pairs": [], "fused": 0, "threads": set()}
    inner_pairs, inner_fused, inner_text = be.engine.contigs_filter_fastq, be.engine.contigs_filter_text, be.engine.filter_text

    def contigs_filter_fastq(*a, **kw):
        seen["threads"].add(threading.get_ident())
        r = inner_pairs(*a, **kw)
        seen["pairs"].append((r.n_built, int(r.n_done)))
        return r

    def contigs_filter_text(*a, **kw):
        seen["threads"].add(threading.get_ident())
        seen["fused"] += 1
        return inner_fused(*a, **kw)

    def filter_text(*a, **kw):
        seen["threads"].add(threading.get_ident())
        return inner_text(*a, **kw)
    be.engine.contigs_filter_fastq, be.engine.contigs_filter_text, be.engine.filter_text = contigs_filter_fastq, contigs_filter_text, filter_text
    return be, seen


def run_cli(out, forward, reverse, pair_index):
    from test_cli_golden import reference_args, same_files
    a = reference_args(paired=True, forward_fastq=forward, reverse_fastq=reverse, output_prefix=out)
    a.device_contigs, a.device_pack, a.device_pair_index = True, True, pair_index
    be, seen = spying_backend()
    log = io.StringIO()
    try:
        assert cli.main(a, backend=be, out=log) == 0
    finally:
        be.engine.close()
    assert "does not apply" not in log.getvalue() and "did not take" not in log.getvalue()
    same_files(out, "paired")                                # tests/golden/reference_test_results/paired.qc.*, byte for byte
    return seen


@pytest.mark.parametrize("form", ("plain", "gz"))
def test_cli_paired_golden_command_with_and_without_the_switch(tmp_path, form):
    f, r = X.golden_texts()
    names = [str(tmp_path / ("in%d.fastq" % k)) + (".gz" if form == "gz" else "") for k in (1, 2)]
    for name, text in zip(names, (f, r)):
        with (gzip.open if form == "gz" else open)(name, "wb") as fh:
            fh.write(text)
    on = run_cli(str(tmp_path / "on"), names[0], names[1], True)
    assert on["fused"] == 0 and sum(c[0] for c in on["pairs"]) == 1000 == sum(c[1] for c in on["pairs"])     # the device built every pair
    off = run_cli(str(tmp_path / "off"), names[0], names[1], False)
    assert off["pairs"] == [] and off["fused"] >= 1


def test_cli_with_six_chunks_makes_every_device_call_on_the_consumer_thread(tmp_path, monkeypatch):
    """Chunks of 192 pairs, six of the golden input, the two files read ahead by a thread each: every call on the context comes
    from the thread that runs cli.main, one text-alone call per chunk and none of today's fused calls."""
    monkeypatch.setattr(cli, "PAIR_CHUNK_READS", 192)
    seen = run_cli(str(tmp_path / "chunks"), os.path.join(GOLD, "test1.fastq.gz"), os.path.join(GOLD, "test2.fastq.bz2"), True)
    assert [c[0] for c in seen["pairs"] if c[0]] == [192] * 5 + [40] and seen["fused"] == 0
    assert seen["threads"] == {threading.get_ident()}
