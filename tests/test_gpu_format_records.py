"""Report lines and the ee suffix formatted on the GPU (include/moira_pb.h: mpb_format_records_host; Engine.format_text(ee=),
Engine.format_report; k_fmt_count, k_fmt_scan, k_fmt_write), and the contigs of mpb_contigs_filter_fastq_host as the resident
text of a generation.  The reference of every case is fastio.format_records (mio_format) / fastio.format_report
(mio_format_report) on the same arguments, byte for byte; the compressed form's is Engine.bgzf_compress of that text.  The
cases are tests/helpers/format_records_inputs.py's, the ones the host lane model runs (tests/test_format_records_model.py)."""
import numpy as np
import pytest

from helpers import collapse_inputs as CI
from helpers import format_inputs as X
from helpers import format_records_inputs as R
from helpers import pair_index_inputs as PI
from moira_amd import engine as E
from moira_amd import fastio as F

pytestmark = pytest.mark.gpu

CASES = R.all_cases()
REFUSED = R.refused_cases()
WANT = {}


def want(c):
    """The reference of a case, computed once."""
    if c["name"] not in WANT:
        WANT[c["name"]] = R.want(c)
    return WANT[c["name"]]


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(0)
    yield e
    e.close()


def fmt(eng, c, **more):
    kw = dict(c["kw"], **more)
    if kw["kind"] != R.REPORT:                               # (mpb_format_records_host, with ee or without)
        return eng.format_text(c["text"], c["idx"], c["sel"], records_entry=True, **kw)
    kw.pop("kind")
    return eng.format_report(c["text"], c["idx"], kw.pop("aux"), c["sel"], **kw)


def named(name):
    return [c for c in CASES if c["name"] == name][0]


# ---- the uploaded form ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_every_case_is_the_host_formatters_bytes(eng, c):
    assert fmt(eng, c) == want(c)


@pytest.mark.parametrize("c,bad", REFUSED, ids=[c["name"] for c, _ in REFUSED])
def test_what_lies_outside_is_a_value_error_with_the_record(eng, c, bad):
    for bgzf in (False, True):
        with pytest.raises(ValueError) as e:
            fmt(eng, c, bgzf=bgzf)
        assert e.value.bad_record == bad
    if c["name"].startswith("ee_outside"):
        assert "ee[%d]" % bad in str(e.value)


def test_window_edges_inside_a_report_line_and_inside_a_suffix(eng, monkeypatch):
    """Windows of 1, 7 and 101 bytes: every line and every suffix of these cases is cut by an edge somewhere."""
    for name, piece in (("count_33_report", 1), ("count_33_report", 7), ("count_33_fasta", 7), ("report_e1_r0_l0", 101), ("report_e1_r1_l0", 1009)):
        c = named(name)
        assert len(want(c)) > 3 * piece
        monkeypatch.setenv("MPB_FORMAT_PIECE_BYTES", str(piece))
        got = fmt(eng, c)
        monkeypatch.delenv("MPB_FORMAT_PIECE_BYTES")
        assert got == want(c), (name, piece)


def test_the_compressed_form_is_bgzf_compress_of_the_text(eng, monkeypatch):
    for name in ("report_e1_r0_l0", "report_e0_r1_l0", "fastq_e1_r0_l1", "qual_e1_r1_l0", "count_1025_report", "count_1_report"):
        c = named(name)
        got = fmt(eng, c, bgzf=True)
        assert got.dtype == np.uint8 and got.tobytes() == eng.bgzf_compress(want(c)), name
    assert len(fmt(eng, named("count_0_report"), bgzf=True)) == 0
    c = named("sel_repeats_report")
    assert len(want(c)) > 65280
    monkeypatch.setenv("MPB_FORMAT_PIECE_BYTES", str(65280 + 77))          # one member per piece
    got = fmt(eng, c, bgzf=True)
    monkeypatch.delenv("MPB_FORMAT_PIECE_BYTES")
    assert got.tobytes() == eng.bgzf_compress(want(c))


def test_without_ee_both_entries_give_the_same_bytes(eng):
    """No ee: Engine.format_text goes through mpb_format_text_host, with records_entry=True through mpb_format_records_host with
    ee and aux NULL -- the path every old call takes through fm_rec_row; a spy on the library sees which entry was called."""
    lib = eng.lib
    seen = []

    class Spy:
        def __getattr__(self, name):
            fn = getattr(lib, name)
            if name.startswith("mpb_format_"):
                seen.append(name)
            return fn
    eng.lib = Spy()
    try:
        for name in ("fasta_e0_r0_l0", "qual_e0_r1_l1", "fastq_e0_r1_l1", "fastq_e0_r0_l0"):
            c = named(name)
            assert "ee" not in c["kw"]
            old = eng.format_text(c["text"], c["idx"], c["sel"], **c["kw"])
            new = eng.format_text(c["text"], c["idx"], c["sel"], records_entry=True, **c["kw"])
            assert old == new == want(c), name
            assert eng.format_text(c["text"], c["idx"], c["sel"], records_entry=True, bgzf=True, **c["kw"]).tobytes() == eng.bgzf_compress(want(c))
    finally:
        eng.lib = lib
    assert seen == ["mpb_format_text_host", "mpb_format_records_host", "mpb_format_records_host"] * 4


# ---- the contig generation --------------------------------------------------------------------------------------------------------

def golden_pairs(n):
    f, r = PI.golden_texts()
    cut = lambda t: b"\n".join(t.split(b"\n")[:4 * n]) + b"\n"
    return cut(f), cut(r)


@pytest.fixture(scope="module")
def texts():
    return golden_pairs(200)


def contigs(eng, texts):
    res = eng.contigs_filter_fastq(*texts)
    assert res.n_built == 200 and res.n_handed_back == 0 and res.filter_error is None
    assert res.resident == eng.resident_text() > 0
    return res


def test_the_contigs_stay_resident_and_every_call_on_them_is_the_host_functions(eng, texts):
    res = contigs(eng, texts)
    n, gen = res.n_built, res.resident
    cbuf, cidx, aux = bytes(res.cbuf), res.cidx, res.aux
    ee = np.where(np.isfinite(res.ee), res.ee, 0.0)
    ri = np.arange(n) * 13
    for sel in (None, np.arange(n)[::-1].copy(), np.arange(1, n, 3)):
        s = np.arange(n) if sel is None else sel
        for kind in X.KINDS:
            assert eng.format_text(idx=cidx, sel=sel, kind=kind, resident=gen) == bytes(F.format_records(cbuf, cidx, s, kind))
            got = eng.format_text(idx=cidx, sel=sel, kind=kind, resident=gen, ee=ee[s], max_len=100, relabel="Seq", relabel_index=ri[s])
            assert got == bytes(F.format_records(cbuf, cidx, s, kind, ee=ee[s], max_len=100, relabel="Seq", relabel_index=ri[s]))
        assert eng.format_report(idx=cidx, sel=sel, resident=gen) == bytes(F.format_report(cbuf, cidx, s, aux))
        assert eng.format_report(idx=cidx, sel=sel, resident=gen, ee=ee[s], relabel="Seq", relabel_index=ri[s]) == bytes(
            F.format_report(cbuf, cidx, s, aux, ee=ee[s], relabel="Seq", relabel_index=ri[s]))
    w = bytes(F.format_report(cbuf, cidx, np.arange(n), aux, ee=ee))
    assert eng.format_report(idx=cidx, resident=gen, ee=ee, bgzf=True).tobytes() == eng.bgzf_compress(w)
    # ... the uploaded form on what came back gives the same lines
    assert eng.format_report(cbuf, cidx, aux, ee=ee) == w
    for max_len in (0, 100):
        h, rep = eng.collapse_text(resident=gen, n=n, max_len=max_len)
        wh, wrep = CI.want(CI.case("contigs", cbuf, cidx, max_len=max_len))
        assert np.array_equal(h, wh) and np.array_equal(rep, wrep)
    assert eng.resident_text() == gen                        # still in force behind all of these


def test_each_contig_call_makes_the_contig_generation_stale(eng, texts):
    ftext, rtext = golden_pairs(30)
    fidx, ridx = F.index(ftext, True, 100)[0], F.index(rtext, True, 100)[0]
    calls = [lambda: eng.contigs_text(ftext, fidx, rtext, ridx), lambda: eng.contigs_filter_text(ftext, fidx, rtext, ridx),
             lambda: eng.contigs_filter_fastq(ftext, rtext)]
    for i, call in enumerate(calls):
        res = contigs(eng, texts)
        later = call()
        now = eng.resident_text()
        assert now != res.resident and now == (getattr(later, "resident", 0) or 0), i
        for stale in (lambda: eng.format_text(idx=res.cidx, resident=res.resident), lambda: eng.format_report(idx=res.cidx, resident=res.resident),
                      lambda: eng.collapse_text(resident=res.resident, n=res.n_built)):
            with pytest.raises(E.NotResident):
                stale()


def test_a_single_end_generation_stays_in_force_behind_the_host_indexed_contig_calls(eng):
    ftext, rtext = golden_pairs(30)
    fidx, ridx = F.index(ftext, True, 100)[0], F.index(rtext, True, 100)[0]
    single = eng.filter_fastq(ftext)
    assert single.resident == eng.resident_text() > 0
    eng.contigs_filter_text(ftext, fidx, rtext, ridx)
    eng.contigs_text(ftext, fidx, rtext, ridx)
    assert eng.resident_text() == single.resident
    assert eng.format_text(idx=single.idx, resident=single.resident) == bytes(F.format_records(ftext, fidx, np.arange(30), F.FMT_FASTQ))
    # ... and it carries no aux: a report call on it is refused as such, not as stale
    with pytest.raises(ValueError) as e:
        eng.format_report(idx=single.idx, resident=single.resident)
    assert not isinstance(e.value, E.NotResident) and "carries no aux" in str(e.value)
    assert eng.resident_text() == single.resident


def test_a_handed_back_pair_leaves_no_generation(eng):
    ftext, rtext = golden_pairs(20)
    lines = ftext.split(b"\n")
    lines[4 * 7 + 1] = b"ACGT" * 96 + b"A"                   # 385 bases: more than the device takes
    lines[4 * 7 + 3] = b"I" * 385
    res = eng.contigs_filter_fastq(b"\n".join(lines), rtext)
    assert res.n_built == 20 and res.n_handed_back == 1 and not res.done[7]
    assert res.resident == 0 and eng.resident_text() == 0
    with pytest.raises(E.NotResident):
        eng.format_report(idx=res.cidx, resident=1)
