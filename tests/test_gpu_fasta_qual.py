"""fasta+qual input on the GPU (include/moira_pb.h: mpb_fasta_qual_index_host, mpb_filter_fasta_qual_host; Engine.fasta_qual_index,
Engine.filter_fasta_qual; the record index's line kernels over both texts, then k_fa_count, k_fa_scan, k_fa_write).  The
reference of every case is fastio.fasta_qual_index (mio_fasta_qual_index) on the same texts and Engine.filter_text(fastq_offset=0)
on what it built, bit for bit; every hand-back must carry its reason, its text and its record.  The cases are
tests/helpers/fasta_qual_inputs.py's, the ones the host lane model runs (tests/test_fasta_qual_lane_model.py)."""
import ctypes as C

import numpy as np
import pytest

from helpers import bgzf_inputs
from helpers import collapse_inputs
from helpers import fasta_qual_inputs as X
from moira_amd import _lib as L
from moira_amd import engine as E
from moira_amd import fastio as F

pytestmark = pytest.mark.gpu

CASES = X.directed_cases()
ENGINE_CASES = [c for c in CASES if c["out_cap"] == 2 * len(c["ftext"]) + 16]       # (the wrapper sizes out itself)
WANT = {}


def want(c):
    """The reference of a case, computed once."""
    if c["name"] not in WANT:
        WANT[c["name"]] = X.want(c)
    return WANT[c["name"]]


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def golden():
    """The golden reads as fasta + qual text, and what the host makes of them."""
    _, f, q = bgzf_inputs.golden_renderings()
    c = X.case("golden", f, q)
    out, idx, fc, qc = X.want(c)
    assert len(idx) == 1000 and (fc, qc) == (len(f), len(q))
    return f, q, out.copy(), idx.copy()


def raw_index(eng, c, rows=None, filt=False):
    """One call of the C entry with the case's own capacities, out and idx filled with guard bytes."""
    rows = min(c["max_records"], len(c["ftext"]) // 2 + 2) if rows is None else rows
    out, idx = np.full(c["out_cap"] + 4, 0xA5, np.uint8), np.full((rows + 1, 6), -7, np.int64)
    n, fc, qc, used, bad = (C.c_int64(-7) for _ in range(5))
    why, which = C.c_int32(-7), C.c_int32(-7)
    a = (eng.ctx, c["ftext"], len(c["ftext"]), c["qtext"], len(c["qtext"]), int(c["final"]), c["max_records"], c["max_len"], out.ctypes.data,
         c["out_cap"], idx.ctypes.data, rows, C.byref(n), C.byref(fc), C.byref(qc), C.byref(used), C.byref(why), C.byref(which), C.byref(bad))
    rc = eng.lib.mpb_fasta_qual_index_host(*a)
    return rc, out, idx, n.value, fc.value, qc.value, used.value, why.value, which.value, bad.value


def same_filter(eng, res, out, idx, max_len=0, **kw):
    ref = eng.filter_text(out, idx, fastq_offset=0, max_len=max_len, **kw) if len(idx) else None
    assert np.array_equal(res.text, out) and np.array_equal(res.idx, idx)
    if ref is None:
        assert len(res.ee) == 0
        return
    assert np.array_equal(res.ee.view(np.uint64), ref.ee.view(np.uint64)) and np.array_equal(res.ns, ref.ns)
    assert np.array_equal(res.passed, ref.passed) and np.array_equal(res.lens, ref.lens) and np.array_equal(res.has_n, ref.has_n)
    assert (res.n_pass, res.n_overflow) == (ref.n_pass, ref.n_overflow)


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_the_index_entry_is_the_hosts_or_hands_back_with_its_reason(eng, c):
    rc, out, idx, n, fc, qc, used, why, which, bad = raw_index(eng, c)
    assert rc == L.OK
    if c["expect"] is not None:
        assert (why, which, bad) == c["expect"]
        return
    wout, widx, wfc, wqc = want(c)
    assert why == 0 and (n, fc, qc, used) == (len(widx), wfc, wqc, len(wout))
    assert np.array_equal(out[:used], wout) and (out[used:] == 0xA5).all()
    assert np.array_equal(idx[:n], widx) and (idx[n:] == -7).all()


SEEDED = {}
SLICES = 4


def seeded_cases():
    """The lane model's 2,000 seeded valid texts and 600 damaged ones, made once."""
    if not SEEDED:
        SEEDED["all"] = X.fuzz_cases() + X.damage_cases()
    return SEEDED["all"]


@pytest.mark.parametrize("part", range(SLICES))
def test_seeded_fuzz_and_damage_are_taken_as_the_host_takes_them_or_handed_back(eng, part):
    """tests/test_fasta_qual_lane_model.py's rule on the kernels: a text that is taken equals the host's; one the host calls
    unsupported is never taken; one the host takes is handed back only under the lanes' documented superset (a quality token of
    more than three digits: TOKEN, in the qual text).  Every valid text is taken.  All 2,600 texts, in four slices."""
    import re
    cases = seeded_cases()
    assert len(cases) == 2600
    taken = back = 0
    for c in cases[part::SLICES]:
        w = X.want(c)
        rc, out, idx, n, fc, qc, used, why, which, bad = raw_index(eng, c)
        assert rc == L.OK, c["name"]
        if why == 0:
            assert w is not None, c["name"]                  # (never taken where the host says unsupported)
            wout, widx, wfc, wqc = w
            assert (n, fc, qc, used) == (len(widx), wfc, wqc, len(wout)), c["name"]
            assert np.array_equal(out[:used], wout) and (out[used:] == 0xA5).all(), c["name"]
            assert np.array_equal(idx[:n], widx) and (idx[n:] == -7).all(), c["name"]
            taken += 1
        else:
            assert not c["name"].startswith("fuzz"), c["name"]
            assert w is None or ((why, which) == (X.TOKEN, 1) and re.search(rb"\d{4,}", c["qtext"])), (c["name"], why, which, bad)
            back += 1
    assert taken >= 500 and back >= 100                      # (2,000 valid texts and the damaged ones the host takes; the rest)


@pytest.mark.parametrize("c", ENGINE_CASES, ids=[c["name"] for c in ENGINE_CASES])
def test_the_wrappers_return_the_hosts_results_and_the_filters(eng, c):
    kw = dict(final=c["final"], max_records=None if c["max_records"] == X.NO_LIMIT else c["max_records"])
    if c["expect"] is not None:
        for call in (lambda: eng.fasta_qual_index(c["ftext"], c["qtext"], **kw),
                     lambda: eng.filter_fasta_qual(c["ftext"], c["qtext"], max_len=c["max_len"], **kw)):
            with pytest.raises(E.NotTaken) as e:
                call()
            why, which, bad = c["expect"]
            assert (e.value.why, e.value.which, e.value.bad_record) == (why, which, None if bad < 0 else bad)
            assert str(e.value) == L.FA_WHY[why]
        return
    wout, widx, wfc, wqc = want(c)
    out, idx, fc, qc = eng.fasta_qual_index(c["ftext"], c["qtext"], **kw)
    assert np.array_equal(out, wout) and np.array_equal(idx, widx) and (fc, qc) == (wfc, wqc)
    res = eng.filter_fasta_qual(c["ftext"], c["qtext"], max_len=c["max_len"], **kw)
    assert (res.f_consumed, res.q_consumed) == (wfc, wqc) and res.resident == eng.resident_text() > 0
    same_filter(eng, res, wout, widx, max_len=c["max_len"])


def test_the_golden_reads_in_one_call_and_in_small_pieces(eng, golden, monkeypatch):
    f, q, out, idx = golden
    res = eng.filter_fasta_qual(f, q)
    same_filter(eng, res, out, idx)
    assert 0 < res.n_pass < 1000
    stride = -(-int(idx[:, F.SEQ_LEN].max()) // 128) * 128
    monkeypatch.setenv("MPB_TEXT_PIECE_BYTES", str(400 * stride))               # 1,000 rows in pieces of 400: three pieces
    pieces = eng.filter_fasta_qual(f, q, max_len=100, poisson=True)
    monkeypatch.delenv("MPB_TEXT_PIECE_BYTES")
    same_filter(eng, pieces, out, idx, max_len=100, poisson=True)
    # the same reads behind the limit and non-final: fewer records, the rest is left to the next call
    part = eng.filter_fasta_qual(f[:len(f) // 2], q, final=False, max_records=700)
    wout, widx, wfc, wqc = X.want(X.case("half", f[:len(f) // 2], q, final=False, max_records=700))
    assert 0 < len(widx) < 700 and (part.f_consumed, part.q_consumed) == (wfc, wqc)
    same_filter(eng, part, wout, widx)


def test_an_index_that_is_too_small_is_asked_again(eng):
    c = [c for c in CASES if c["name"] == "tile_edge"][0]
    rc, out, idx, n, *_ = raw_index(eng, c, rows=109)
    assert (rc, n) == (L.E_INVALID, 110) and (idx == -7).all() and (out == 0xA5).all()
    assert b"idx_cap_rows" in eng.lib.mpb_last_error()
    rc, out, idx, n, fc, qc, used, why, which, bad = raw_index(eng, c, rows=110)
    assert (rc, n, why) == (L.OK, 110, 0) and np.array_equal(idx[:n], want(c)[1])
    # through the wrapper: more records than its guess of 64 bytes each
    recs = [(b"%d" % i, b"AC", [i % 200, 3]) for i in range(3000)]
    f, q = X.render(recs)
    assert len(f) // 64 + 64 < 3000
    wout, widx, _, _ = X.want(X.case("many", f, q))
    out, idx, fc, qc = eng.fasta_qual_index(f, q)
    assert len(idx) == 3000 and np.array_equal(out, wout) and np.array_equal(idx, widx) and (fc, qc) == (len(f), len(q))


def test_what_lies_behind_the_texts_on_the_device_changes_nothing(eng):
    """The blocks are the context's and keep what earlier calls left: the same texts behind longer texts of digits, of line ends
    and of high bytes -- whatever then lies between text_bytes and the end of its last 16-byte word, and behind it."""
    f, q = X.render(X.straddle_records(), last_eol=False)
    while not (len(f) % 16 and len(q) % 16):                 # (both texts end inside a word)
        f, q = b">lead\nAC\n" + f, b">lead\n7 8\n" + q
    c = X.case("padding", f, q)
    wout, widx, wfc, wqc = X.want(c)
    assert len(widx) >= 16 and (wfc, wqc) == (len(f), len(q))
    for fill in (b"9", b"\n", b"\r", b" ", b"\x80", b">"):
        try:
            eng.fasta_qual_index(fill * (len(c["ftext"]) + 64), fill * (len(c["qtext"]) + 64))
        except E.NotTaken:
            pass
        out, idx, fc, qc = eng.fasta_qual_index(c["ftext"], c["qtext"])
        assert np.array_equal(out, wout) and np.array_equal(idx, widx) and (fc, qc) == (wfc, wqc), fill


def test_format_text_takes_the_slots_by_resident(eng, golden):
    f, q, out, idx = golden
    res = eng.filter_fasta_qual(f, q)
    gen = res.resident
    assert gen == eng.resident_text() > 0
    n = len(idx)
    for sel in (None, np.arange(1, n, 3)):
        rows = np.arange(n) if sel is None else sel
        for kind in (F.FMT_FASTA, F.FMT_QUAL, F.FMT_FASTQ):
            kw = dict(fastq_offset=0, out_offset=33, max_len=0 if sel is None else 100)
            w = bytes(F.format_records(out, idx, rows, kind, **kw))
            assert eng.format_text(idx=res.idx, sel=sel, kind=kind, resident=gen, **kw) == w
            z = eng.format_text(idx=res.idx, sel=sel, kind=kind, resident=gen, bgzf=True, **kw)
            assert z.tobytes() == eng.bgzf_compress(w)
            import zlib
            text, at, blob = b"", 0, z.tobytes()
            while at < len(blob):
                size = int.from_bytes(blob[at + 16:at + 18], "little") + 1
                text += zlib.decompress(blob[at + 18:at + size - 8], -15)
                at += size
            assert text == w
    assert eng.resident_text() == gen                      # (format calls leave the generation in force)


def test_collapse_text_takes_the_slots_by_resident(eng, golden):
    f, q, out, idx = golden
    for max_len in (0, 100):
        res = eng.filter_fasta_qual(f, q)
        h, rep = collapse_inputs.want(collapse_inputs.case("golden", out.tobytes(), idx, max_len=max_len))
        assert np.array_equal(h, np.array(F.py2_hashes(out, idx, max_len), np.uint64))
        got = eng.collapse_text(resident=res.resident, n=len(idx), max_len=max_len)
        assert np.array_equal(got[0], h) and np.array_equal(got[1], rep)
        assert len(set(rep.tolist())) < len(idx)


def test_a_later_call_makes_the_generation_stale(eng, golden):
    f, q, out, idx = golden
    first = eng.filter_fasta_qual(f, q)
    second = eng.filter_fasta_qual(f, q)
    assert second.resident == first.resident + 1
    with pytest.raises(E.NotResident):
        eng.format_text(idx=first.idx, resident=first.resident)
    calls = [lambda: eng.fasta_qual_index(f, q), lambda: eng.fasta_qual_index(f, q[:-7]), lambda: eng.filter_fasta_qual(b">a\nAC\n", b">b\n1 2\n"),
             lambda: eng.filter_fasta_qual(f, q)]
    for i, call in enumerate(calls):
        res = eng.filter_fasta_qual(f, q)
        assert res.resident == eng.resident_text() > 0
        try:
            later = call()
        except E.NotTaken:
            later = None
        now = eng.resident_text()
        assert now != res.resident and (now == 0 or now == getattr(later, "resident", None)), i
        with pytest.raises(E.NotResident):
            eng.format_text(idx=res.idx, resident=res.resident)
        with pytest.raises(E.NotResident):
            eng.collapse_text(resident=res.resident, n=len(res.idx))


def test_the_three_kernels_are_timed_in_the_rows_slot(eng, golden):
    f, q, out, idx = golden
    eng.timing(True)
    try:
        eng.timing_reset()
        eng.fasta_qual_index(f, q)
        t = eng.kernel_times()
        busy = {name for name, (_, n) in t.items() if n}
        assert busy == {"fq_lines", "fq_scan", "fq_starts", "fq_rows"} and t["fq_rows"][1] == 1 and t["fq_rows"][0] > 0
    finally:
        eng.timing(False)
