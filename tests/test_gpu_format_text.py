"""Output records formatted on the GPU (include/moira_pb.h: mpb_format_text_host; Engine.format_text; k_fmt_count, k_fmt_scan,
k_fmt_write).  The reference of every case is fastio.format_records (mio_format) on the same arguments, byte for byte; the
compressed form's is Engine.bgzf_compress of that text, and every member must inflate with zlib to its slice of it.  The cases
are tests/helpers/format_inputs.py's, the ones the host lane model runs (tests/test_format_lane_model.py)."""
import ctypes as C
import struct
import zlib

import numpy as np
import pytest

from helpers import format_inputs as X
from moira_amd import _lib as L
from moira_amd import engine as E
from moira_amd import fastio as F

pytestmark = pytest.mark.gpu

CASES = X.all_cases() + [X.fasta_ignores_quality_columns()]
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
    text = X.golden_text()
    return text, F.index(text, True, 1 << 20)[0].copy()


def fmt(eng, c, **more):
    return eng.format_text(c["text"], c["idx"], c["sel"], **dict(c["kw"], **more))


def members(blob):
    """The BGZF members of a stream without end marker -> their texts, CRC-32 and ISIZE checked."""
    blob, out, at = bytes(blob), [], 0
    while at < len(blob):
        assert blob[at:at + 4] == b"\x1f\x8b\x08\x04" and blob[at + 12:at + 14] == b"BC"
        size = struct.unpack_from("<H", blob, at + 16)[0] + 1
        text = zlib.decompress(blob[at + 18:at + size - 8], -15)
        crc, isize = struct.unpack_from("<II", blob, at + size - 8)
        assert crc == zlib.crc32(text) and isize == len(text)
        out.append(text)
        at += size
    assert at == len(blob)
    return out


def check_compressed(eng, got, text):
    assert got.dtype == np.uint8 and got.tobytes() == eng.bgzf_compress(text)
    ms = members(got)
    assert ms == [text[at:at + L.BGZF_DATA] for at in range(0, len(text), L.BGZF_DATA)]
    return ms


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_every_case_is_fastio_formats_bytes(eng, c):
    assert fmt(eng, c) == want(c)


def test_a_byte_below_the_offset_stays_with_equal_offsets_only(eng):
    text, idx = X.build([(b"r", b"ACGT", bytes([32, 33, 34, 32]))])
    for out_off in (33, 64):
        c = X.case("below", text, idx, kind=F.FMT_FASTQ, fastq_offset=33, out_offset=out_off)
        assert fmt(eng, c) == X.want(c)


@pytest.mark.parametrize("c,bad", X.damaged_cases(), ids=[c["name"] for c, _ in X.damaged_cases()])
def test_damaged_rows_are_value_errors_with_the_record(eng, c, bad):
    with pytest.raises(ValueError) as e:
        fmt(eng, c)
    assert e.value.bad_record == bad
    with pytest.raises(ValueError) as e:
        fmt(eng, c, bgzf=True)
    assert e.value.bad_record == bad


def raw(eng, c, cap, bgzf=0):
    """One call of the C entry with an output of `cap` bytes behind which four guard bytes lie -> (rc, out, bytes, needed, bad)."""
    idx = c["idx"]
    out = np.full(cap + 4, 0xA5, np.uint8)
    got, needed, bad = C.c_int64(-7), C.c_int64(-7), C.c_int64(-7)
    rc = eng.lib.mpb_format_text_host(eng.ctx, c["text"], len(c["text"]), idx.ctypes.data, len(idx), 0, None, len(idx), c["kw"]["kind"], 33, 33,
                                      1, 0, None, None, None, 0, None, bgzf, out.ctypes.data, cap, C.byref(got), C.byref(needed),
                                      C.byref(bad), None)
    return rc, out, got.value, needed.value, bad.value


def test_an_output_one_byte_short_says_what_is_needed_and_asking_again_succeeds(eng):
    c = [c for c in CASES if c["name"] == "count_257_qual"][0]
    w = want(c)
    rc, out, got, needed, bad = raw(eng, c, len(w) - 1)
    assert (rc, got, needed, bad) == (L.E_INVALID, 0, len(w), -1) and (out == 0xA5).all()
    rc, out, got, needed, bad = raw(eng, c, needed)
    assert (rc, got, needed, bad) == (L.OK, len(w), len(w), -1) and out[:got].tobytes() == w and (out[got:] == 0xA5).all()
    # the compressed form: the bound of the text that is needed
    cap = C.c_int64()
    L.check(eng.lib.mpb_bgzf_bound(len(w), C.byref(cap)))
    rc, out, got, needed, bad = raw(eng, c, cap.value - 1, bgzf=1)
    assert (rc, got, needed) == (L.E_INVALID, 0, len(w)) and (out == 0xA5).all()
    rc, out, got, needed, bad = raw(eng, c, cap.value, bgzf=1)
    assert rc == L.OK and needed == len(w) and out[:got].tobytes() == eng.bgzf_compress(w) and (out[got:] == 0xA5).all()


def test_a_damaged_row_writes_nothing(eng):
    c, bad = X.damaged_cases()[0]
    rc, out, got, needed, b = raw(eng, c, 1 << 16)
    assert (rc, got, b) == (L.E_INVALID, 0, bad) and (out == 0xA5).all()


def test_three_pieces_give_the_same_bytes_in_both_forms(eng, golden, monkeypatch):
    text, idx = golden
    for kind in (F.FMT_FASTQ, F.FMT_QUAL):
        w = bytes(F.format_records(text, idx, np.arange(len(idx)), kind))
        whole = eng.format_text(text, idx, kind=kind, bgzf=True)
        monkeypatch.setenv("MPB_FORMAT_PIECE_BYTES", str(len(w) // 3 + 1))       # windows that end inside records
        assert eng.format_text(text, idx, kind=kind) == w
        monkeypatch.setenv("MPB_FORMAT_PIECE_BYTES", str((len(w) // L.BGZF_DATA // 3 + 1) * L.BGZF_DATA + 77))
        assert -(-len(w) // ((len(w) // L.BGZF_DATA // 3 + 1) * L.BGZF_DATA)) == 3
        pieces = eng.format_text(text, idx, kind=kind, bgzf=True)
        monkeypatch.delenv("MPB_FORMAT_PIECE_BYTES")
        assert np.array_equal(pieces, whole)
        check_compressed(eng, pieces, w)
    monkeypatch.setenv("MPB_FORMAT_PIECE_BYTES", "1")        # (a window smaller than any record; members of their own pieces)
    c = [c for c in CASES if c["name"] == "count_63_qual"][0]
    assert fmt(eng, c) == want(c)
    check_compressed(eng, fmt(eng, c, bgzf=True), want(c))


# ---- the resident form ------------------------------------------------------------------------------------------------------------

def resident_same(eng, res, text, **kw):
    idx = F.index(text, True, 1 << 20)[0]
    assert np.array_equal(res.idx, idx) and res.resident == eng.resident_text() > 0
    n = len(idx)
    for sel in (None, np.arange(n)[::-1], np.arange(1, n, 3)):
        for kind in X.KINDS:
            got = eng.format_text(idx=res.idx, sel=sel, kind=kind, resident=res.resident, **kw)
            assert got == bytes(F.format_records(text, idx, np.arange(n) if sel is None else sel, kind, **kw))


def test_resident_behind_filter_fastq(eng, golden):
    text = X.golden_text(300)
    res = eng.filter_fastq(text)
    resident_same(eng, res, text)
    ri = np.arange(len(res.idx)) * 37
    got = eng.format_text(idx=res.idx, kind=F.FMT_FASTQ, resident=res.resident, max_len=100, relabel="Seq", relabel_index=ri)
    assert got == bytes(F.format_records(text, res.idx, np.arange(len(res.idx)), F.FMT_FASTQ, max_len=100, relabel="Seq", relabel_index=ri))
    w = bytes(F.format_records(text, res.idx, np.arange(len(res.idx)), F.FMT_FASTQ))
    check_compressed(eng, eng.format_text(idx=res.idx, kind=F.FMT_FASTQ, resident=res.resident, bgzf=True), w)


def test_resident_behind_filter_bgzf_fastq_with_a_carry(eng):
    from helpers import bgzf_fastq_inputs as M
    text = X.golden_text(300)
    cut = 1234                                               # the carry ends inside a record
    batch = M.batch_of(M.cut(text[cut:], 20000))
    res = eng.filter_bgzf_fastq(*batch, carry=text[:cut], text=False)
    assert res.text is None
    resident_same(eng, res, text)


def test_a_later_call_makes_the_generation_stale(eng):
    from helpers import bgzf_fastq_inputs as M
    text = X.golden_text(50)
    idx = F.index(text, True, 1000)[0]
    first = eng.filter_fastq(text)
    second = eng.filter_fastq(text)
    assert second.resident == first.resident + 1
    with pytest.raises(E.NotResident):
        eng.format_text(idx=first.idx, resident=first.resident)
    assert eng.format_text(idx=second.idx, resident=second.resident) == bytes(F.format_records(text, idx, np.arange(50), F.FMT_FASTQ))
    # a format call, uploaded or resident, leaves the resident text in force
    assert eng.format_text(text, idx, kind=F.FMT_QUAL) == bytes(F.format_records(text, idx, np.arange(50), F.FMT_QUAL))
    assert eng.resident_text() == second.resident
    # every call the header lists as invalidating: the generation is none behind it, whatever the call made of its text
    calls = [lambda: eng.fastq_index(text), lambda: eng.filter_fastq(b"@r\nAC\r+\nII\n"), lambda: eng.filter_fastq(text),
             lambda: eng.filter_bgzf_fastq(*M.batch_of(M.cut(text, 5000))), lambda: eng.contigs_filter_fastq(text, text)]
    for i, call in enumerate(calls):
        res = eng.filter_fastq(text)
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
        eng.format_text(idx=idx, resident=12345)


def raw_resident(eng, gen, n, cap, sel=None, relabel=None, relabel_index=None, labels=None, label_id=None, bgzf=0, kind=2):
    """One call of the C entry in the resident form, its output filled with guard bytes -> (rc, out, bytes, needed, bad)."""
    nsel = n if sel is None else len(sel)
    keep = [None if a is None else np.ascontiguousarray(a, t) for a, t in ((sel, np.int64), (relabel_index, np.int64), (label_id, np.int32))]
    ptr = lambda a: None if a is None else a.ctypes.data
    enc = [s.encode() for s in labels or []]
    lab = (C.c_char_p * max(len(enc), 1))(*enc)
    out = np.full(cap + 4, 0xA5, np.uint8)
    got, needed, bad = C.c_int64(-7), C.c_int64(-7), C.c_int64(-7)
    rc = eng.lib.mpb_format_text_host(eng.ctx, None, 0, None, n, gen, ptr(keep[0]), nsel, kind, 33, 33, 1, 0, relabel, ptr(keep[1]),
                                      C.cast(lab, C.c_void_p) if labels else None, len(enc), ptr(keep[2]), bgzf, out.ctypes.data, cap,
                                      C.byref(got), C.byref(needed), C.byref(bad), None)
    return rc, out, got.value, needed.value, bad.value


def test_the_kernels_refuse_what_a_resident_call_selects_wrongly(eng):
    """The resident form validates nothing on the host: sel, relabel_index and label_id reach k_fmt_count as the caller gave them.
    The first offending k comes back (an atomic min: two offenders, the later one first in memory order of the grid or not), nothing
    is written in either form, and the generation stays in force."""
    text = X.golden_text(300)
    res = eng.filter_fastq(text)
    n, gen = len(res.idx), res.resident
    assert n == 300 and gen > 0
    ok = np.arange(n)

    def damaged(at, value, base=ok):
        a = base.copy()
        a[at] = value
        return a
    two = damaged(9, -3, damaged(270, n))                    # two offenders, workgroups apart: the minimum matters
    cases = [(dict(sel=damaged(5, n)), 5), (dict(sel=damaged(5, -1)), 5), (dict(sel=damaged(299, 1 << 40)), 299), (dict(sel=two), 9),
             (dict(sel=two[::-1].copy()), 29),
             (dict(relabel=b"S", relabel_index=damaged(7, -1)), 7),
             (dict(relabel=b"S", relabel_index=damaged(7, -1, damaged(200, -5))), 7),
             (dict(labels=X.LABELS[:3], label_id=damaged(3, 3, np.zeros(n, np.int64))), 3),
             (dict(labels=X.LABELS[:3], label_id=damaged(250, 100, np.full(n, -1))), 250)]
    for kw, bad in cases:
        for bgzf in (0, 1):
            rc, out, got, needed, b = raw_resident(eng, gen, n, 1 << 20, bgzf=bgzf, **kw)
            assert (rc, got, b) == (L.E_INVALID, 0, bad) and (out == 0xA5).all(), (kw.keys(), bad, bgzf)
            assert b"the kernel refused selected record %d" % bad in eng.lib.mpb_last_error()
        assert eng.resident_text() == gen
    # ... and through the wrapper: ValueError with the record
    for kw, bad in ((dict(sel=two), 9), (dict(relabel="S", relabel_index=damaged(7, -1)), 7),
                    (dict(labels=X.LABELS[:3], label_id=damaged(3, 3, np.zeros(n, np.int64))), 3)):
        for bgzf in (False, True):
            with pytest.raises(ValueError) as e:
                eng.format_text(idx=res.idx, resident=gen, bgzf=bgzf, **kw)
            assert e.value.bad_record == bad
    # the generation is still in force, and the same arguments mended are taken
    assert eng.resident_text() == gen
    rc, out, got, needed, b = raw_resident(eng, gen, n, 1 << 20, sel=ok[::-1].copy(), relabel=b"S", relabel_index=ok)
    w = bytes(F.format_records(text, res.idx, ok[::-1], F.FMT_FASTQ, relabel="S", relabel_index=ok))
    assert (rc, got, needed, b) == (L.OK, len(w), len(w), -1) and out[:got].tobytes() == w and (out[got:] == 0xA5).all()
    assert eng.format_text(idx=res.idx, resident=gen, relabel=b"S", relabel_index=ok) == bytes(
        F.format_records(text, res.idx, ok, F.FMT_FASTQ, relabel="S", relabel_index=ok))       # (a bytes relabel is taken as well)


# ---- the compressed form ----------------------------------------------------------------------------------------------------------

def test_compressed_empty_selection_has_no_member(eng, golden):
    text, idx = golden
    got = eng.format_text(text, idx, sel=np.zeros(0, np.int64), bgzf=True)
    assert got.dtype == np.uint8 and len(got) == 0 and eng.bgzf_compress(b"") == b""


@pytest.mark.parametrize("total", [L.BGZF_DATA, L.BGZF_DATA + 1])
def test_compressed_text_of_one_member_and_one_byte_more(eng, total):
    rng = np.random.default_rng(3)
    recs = [(b"r%d" % i, X.bases(rng, 6000), X.quals(rng, 6000)) for i in range(10)]
    text, idx = X.build(recs)
    size = len(F.format_records(text, idx, np.arange(10), F.FMT_FASTA))
    last = 6000 + total - size
    recs[-1] = (b"r9", X.bases(rng, last), X.quals(rng, last))
    text, idx = X.build(recs)
    w = bytes(F.format_records(text, idx, np.arange(10), F.FMT_FASTA))
    assert len(w) == total
    assert len(check_compressed(eng, eng.format_text(text, idx, kind=F.FMT_FASTA, bgzf=True), w)) == (1 if total == L.BGZF_DATA else 2)


def test_compressed_golden_reads_in_all_kinds(eng, golden):
    text, idx = golden
    for kind in X.KINDS:
        w = bytes(F.format_records(text, idx, np.arange(len(idx)), kind))
        check_compressed(eng, eng.format_text(text, idx, kind=kind, bgzf=True), w)
        st = eng.bgzf_stats()
        assert st["members"] == -(-len(w) // L.BGZF_DATA) and st["dynamic"] >= 1


def test_the_three_kernels_are_timed_in_the_pack_slot_alone(eng, golden):
    text, idx = golden
    eng.timing(True)
    try:
        eng.timing_reset()
        eng.format_text(text, idx, kind=F.FMT_QUAL)
        t = eng.kernel_times()
        assert t["pack_text"][1] == 2 and t["pack_text"][0] > 0                     # count + scan, write
        assert all(n == 0 for name, (_, n) in t.items() if name != "pack_text")
        eng.timing_reset()
        eng.format_text(text, idx, kind=F.FMT_QUAL, bgzf=True)
        t = eng.kernel_times()
        busy = {name for name, (_, n) in t.items() if n}
        assert busy == {"pack_text", "bgzf_deflate", "bgzf_scan", "bgzf_frame"}
    finally:
        eng.timing(False)
