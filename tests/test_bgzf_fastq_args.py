"""What of the fused BGZF FASTQ call needs no device: the argument checks of mpb_crc32_ranges_host / mpb_filter_bgzf_fastq_host
(made before the context is looked at), fastio.GzipReader's split into "scan a batch" and "inflate a scanned batch"
(read_members / inflate_batch beside an unchanged read), the producer's items (cli._read_members) and the consumer's side
(cli._DeviceIndexer.take_members) against a fake engine whose filter_bgzf_fastq is zlib + fastio.index + a stub.  The lane code
on the host: tests/test_crc_lane_model.py; the kernels: tests/test_gpu_crc32.py, tests/test_gpu_bgzf_fastq.py."""
import ctypes as C
import gzip
import io
import os
import types

import numpy as np
import pytest

from helpers import bgzf_fastq_inputs as M
from helpers import fastq_index_texts as X
from helpers import inflate_inputs as I
from moira_amd import _lib as L
from moira_amd import cli
from moira_amd import engine as E
from moira_amd import fastio as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


# ---- the C ABI's argument checks ---------------------------------------------------------------------------------------------

def test_the_entries_are_declared_and_no_constant_moved():
    hdr = open(os.path.join(ROOT, "include", "moira_pb.h")).read()
    assert "int mpb_crc32_ranges_host(" in hdr and "int mpb_filter_bgzf_fastq_host(" in hdr
    assert "mpb_crc32_ranges_host" in L.PROTOTYPES and "mpb_filter_bgzf_fastq_host" in L.PROTOTYPES
    assert len(L.PROTOTYPES["mpb_crc32_ranges_host"][1]) == 7 and len(L.PROTOTYPES["mpb_filter_bgzf_fastq_host"][1]) == 35
    assert "#define MPB_K_COUNT     22" in hdr and len(L.FQ_WHY) == 5 and len(L.BGZF_WHY) == 14       # no kernel id, no reason added
    lib = L.load()
    assert lib.mpb_crc32_ranges_host and lib.mpb_filter_bgzf_fastq_host
    e = E.MembersNotTaken(1, np.array([1, 0], np.uint8), np.array([0, 13], np.uint8))
    assert (e.first, str(e)) == (1, "member 1: crc")
    assert issubclass(E.BgzfFastqFilterResult, E.FastqFilterResult)


def crc_call(text=b"abcdef", text_bytes=None, offs=(0, 2), lens=(6, 3), n=None, null=()):
    lib = L.load()
    o, l = np.array(offs, np.int64), np.array(lens, np.int32)
    out = np.zeros(max(len(o), 1), np.uint32)
    ptr = lambda name, v: None if name in null else v
    rc = lib.mpb_crc32_ranges_host(None, ptr("text", text), len(text) if text_bytes is None else text_bytes, ptr("offs", o.ctypes.data),
                                   ptr("lens", l.ctypes.data), len(o) if n is None else n, ptr("out", out.ctypes.data))
    return rc, lib.mpb_last_error().decode()


def test_crc_argument_errors_are_invalid_with_or_without_a_device():
    rc, msg = crc_call()
    assert rc == L.E_INVALID and "mpb_crc32_ranges_host: ctx is NULL" in msg       # good arguments: only the context is missing
    rc, msg = crc_call(offs=(), lens=())
    assert rc == L.E_INVALID and "ctx is NULL" in msg
    for kw in (dict(n=-1), dict(text_bytes=-1), dict(null=("text",)), dict(null=("offs",)), dict(null=("lens",)), dict(null=("out",))):
        rc, msg = crc_call(**kw)
        assert rc == L.E_INVALID and "mpb_crc32_ranges_host: bad arguments" in msg, kw
    for kw, k in ((dict(offs=(0, 4), lens=(6, 3)), 1), (dict(offs=(-1, 0), lens=(1, 1)), 0), (dict(offs=(0, 0), lens=(1, -1)), 1),
                  (dict(offs=(7,), lens=(0,)), 0), (dict(text=bytes(70000), offs=(0,), lens=(65537,)), 0)):
        rc, msg = crc_call(**kw)
        assert rc == L.E_INVALID and "mpb_crc32_ranges_host: range %d " % k in msg, (kw, msg)
    assert "1 GiB" in crc_call(text_bytes=(1 << 30) + 1)[1]


def fused_call(members=None, carry=b"", carry_len=None, n_members=None, in_len=None, out_offs=None, final=1, max_records=10, max_len=0,
               text_cap=None, cap=11, offset=33, params=E.Engine.params(), null=()):
    lib = L.load()
    members = [I.neighbour()[0]] if members is None else members
    data, offs, sizes, oo = M.batch_of(members)
    oo = oo if out_offs is None else np.array(out_offs, np.int64)
    m = len(members) if n_members is None else n_members
    total = len(carry) + int(oo[-1])
    text = np.zeros(max(total, 1), np.uint8)
    idx = np.zeros((max(cap, 1), 6), np.int64)
    ee, ns, ps = np.zeros(max(cap, 1)), np.zeros(max(cap, 1), np.int32), np.zeros(max(cap, 1), np.uint8)
    done, mwhy = np.zeros(max(m, 1), np.uint8), np.zeros(max(m, 1), np.uint8)
    fb, n, consumed, bad, why, badrec = C.c_int64(-7), C.c_int64(-7), C.c_int64(-7), C.c_int32(-7), C.c_int32(-7), C.c_int64(5)
    ptr = lambda name, v: None if name in null else v
    rc = lib.mpb_filter_bgzf_fastq_host(
        None, ptr("carry", carry), len(carry) if carry_len is None else carry_len, ptr("in", data.ctypes.data),
        len(data) if in_len is None else in_len, ptr("offs", offs.ctypes.data), ptr("sizes", sizes.ctypes.data),
        ptr("out_offs", oo.ctypes.data), m, final, max_records, max_len, ptr("text", text.ctypes.data),
        len(text) if text_cap is None else text_cap, ptr("done", done.ctypes.data), ptr("mwhy", mwhy.ctypes.data),
        ptr("first_back", C.byref(fb)), None, ptr("idx", idx.ctypes.data), cap, ptr("n", C.byref(n)), ptr("consumed", C.byref(consumed)),
        ptr("bad", C.byref(bad)), ptr("why", C.byref(why)), offset, 0, C.byref(params) if params is not None else None, 0,
        ptr("ee", ee.ctypes.data), ptr("ns", ns.ctypes.data), ptr("pass", ps.ctypes.data), None, None, None, C.byref(badrec))
    return rc, lib.mpb_last_error().decode(), badrec.value


def test_fused_argument_errors_are_invalid_with_or_without_a_device():
    rc, msg, badrec = fused_call()
    assert rc == L.E_INVALID and "mpb_filter_bgzf_fastq_host: ctx is NULL" in msg and badrec == -1     # good arguments
    for kw in (dict(members=[]), dict(members=[], carry=b"@r\nAC"), dict(null=("text",)), dict(null=("mwhy",)),
               dict(null=("carry",)), dict(members=[], null=("in", "offs", "sizes", "done"))):
        rc, msg, _ = fused_call(**kw)
        assert rc == L.E_INVALID and "ctx is NULL" in msg, (kw, msg)                 # what may be NULL, and no member at all
    bad = [dict(null=(name,)) for name in ("in", "offs", "sizes", "out_offs", "done", "first_back", "idx", "n", "consumed", "bad", "why",
                                             "ee", "ns", "pass")]
    bad += [dict(carry=b"@r", null=("carry",)), dict(carry_len=-1), dict(in_len=-1), dict(n_members=-1), dict(max_records=-1),
            dict(max_len=-1), dict(text_cap=-1), dict(cap=0)]
    for kw in bad:
        rc, msg, _ = fused_call(**kw)
        assert rc == L.E_INVALID and "mpb_filter_bgzf_fastq_host: bad arguments" in msg, (kw, msg)
    rc, msg, _ = fused_call(members=[], carry_len=(1 << 30) + 1, carry=b"x")
    assert rc == L.E_INVALID and "mpb_filter_bgzf_fastq_host: text of" in msg and "1 GiB" in msg
    rc, msg, _ = fused_call(carry_len=1 << 29, carry=b"x", out_offs=[0, (1 << 29) + 1], null=("text",))
    assert rc == L.E_INVALID and "1 GiB" in msg                                     # carry + members together
    rc, msg, _ = fused_call(text_cap=10)
    assert rc == L.E_INVALID and "mpb_filter_bgzf_fastq_host: text_cap 10 is below the" in msg
    rc, msg, _ = fused_call(text_cap=10, null=("text",))                            # ... which counts only with a text_out
    assert "ctx is NULL" in msg
    assert "mpb_filter_bgzf_fastq_host: fastq_offset 256" in fused_call(offset=256)[1] and "fastq_offset -1" in fused_call(offset=-1)[1]
    assert "params is NULL" in fused_call(params=None)[1]
    rc, msg, _ = fused_call(out_offs=[5, 805])
    assert rc == L.E_INVALID and "out_offs must start at 0" in msg
    rc, msg, _ = fused_call(in_len=10)                                              # the rows' own argument check, before the context
    assert rc == L.E_INVALID and "mpb_bgzf_member_rows: member 0" in msg


# ---- GzipReader: read() as before, read_members + inflate_batch beside it --------------------------------------------------------

def reader(blob, **kw):
    return F.GzipReader(io.BytesIO(blob), **kw)


def read_all(r, n=1 << 25):
    out = []
    while True:
        d = r.read(n)
        if not d:
            return b"".join(out)
        out.append(d)


def members_then_text(blob, n=1 << 25, **kw):
    """Everything read_members yields, inflated by inflate_batch, then what read() still serves -> (text, batches)."""
    r = reader(blob, **kw)
    out, batches = [], 0
    while True:
        b = r.read_members(n)
        if b is None:
            break
        assert b[0].dtype == np.uint8 and len(b[1]) == len(b[2]) == len(b[3]) - 1 >= 1 and b[3][0] == 0
        assert int(b[1][-1]) + int(b[2][-1]) == len(b[0])
        batches += 1
        out.append(r.inflate_batch(b))
    assert r.read_members(n) is None
    out.append(read_all(r, n))
    r.close()
    return b"".join(out), batches


def bgzf_files():
    gold = open(os.path.join(GOLD, "test1.fastq.gz"), "rb").read()
    text = gzip.decompress(gold)
    valid = [I.frame(s, t) for _, s, t, _ in I.zlib_members()[:6] + I.crafted_valid()]
    return [("golden", gold), ("golden_bgzf", cli.bgzf_compress(text) + cli.BGZF_EOF), ("members", b"".join(valid)),
            ("small_members", b"".join(M.cut(text[:30000], 700)))]


@pytest.mark.parametrize("threads", [1, 4])
def test_read_returns_what_gzip_returns(threads):
    for name, blob in bgzf_files():
        want = gzip.decompress(blob)
        for n in (1 << 25, 100000, 4096):
            r = reader(blob, threads=threads)
            assert read_all(r, n) == want, (name, n)
            r.close()


def test_read_members_then_inflate_batch_gives_the_same_bytes():
    for name, blob in bgzf_files():
        want = gzip.decompress(blob)
        is_bgzf = name != "golden" or blob[12:14] == b"BC"
        for n in (1 << 25, 50000):
            got, batches = members_then_text(blob, n, threads=4)
            assert got == want, (name, n)
            assert (batches >= 1) == is_bgzf, name
        got, batches = members_then_text(blob, threads=1)      # one thread, no inflater: the reader does not look for members
        assert got == want and batches == 0


def test_a_plain_gzip_file_gives_none_at_once_and_read_serves_it():
    text = M.golden_text(50)
    blob = gzip.compress(text)
    r = reader(blob, threads=4)
    assert r.read_members() is None and r.bgzf is False
    assert read_all(r) == text
    r.close()


def test_zero_padding_and_a_truncated_member_end_as_they_did():
    text = M.golden_text(50)
    blob = b"".join(M.cut(text, 3000))
    got, batches = members_then_text(blob + bytes(700), threads=4)
    assert got == text and batches == 1
    r = reader(blob + bytes(700), threads=4)
    assert read_all(r) == text
    r.close()
    cutoff = blob[:-11]
    errs = []
    for how in ("read", "members"):
        with pytest.raises(OSError) as e:
            if how == "read":
                r = reader(cutoff, threads=4)
                read_all(r)
            else:
                members_then_text(cutoff, threads=4)
        errs.append(str(e.value))
    assert errs[0] == errs[1] and errs[0].startswith("gzip input: ")


def test_a_corrupt_member_raises_the_same_error_either_way():
    good, _ = I.neighbour()
    wrong = [m for name, m, why in I.crafted_invalid() if name == "wrong_crc"][0]
    blob = good + good + wrong + good
    errs = []
    for how in ("read", "members"):
        with pytest.raises(OSError) as e:
            if how == "read":
                read_all(reader(blob, threads=4))
            else:
                members_then_text(blob, threads=4)
        errs.append(str(e.value))
    assert errs[0] == errs[1] and "BGZF block 2" in errs[0]


def test_the_producer_holds_one_batch_back_to_know_the_end():
    text = M.golden_text(60)
    blob = b"".join(M.cut(text, 2000))
    items = list(cli._read_members(reader(blob, threads=4), 6000))
    assert len(items) > 2 and all(isinstance(i, cli._DeferredMembers) for i in items)
    assert [i.eof for i in items] == [False] * (len(items) - 1) + [True]
    assert b"".join(M.inflated(i.batch) for i in items) == text
    plain = list(cli._read_members(reader(gzip.compress(text), threads=4), 6000))
    assert all(isinstance(i, cli._DeferredBlock) for i in plain) and plain[-1].eof and plain[-1].data == b""
    assert b"".join(i.data for i in plain) == text
    mixed = list(cli._read_members(reader(blob + gzip.compress(text), threads=4), 1 << 20))     # BGZF, then one plain member
    assert isinstance(mixed[0], cli._DeferredMembers) and not mixed[0].eof and isinstance(mixed[-1], cli._DeferredBlock)
    assert M.inflated(mixed[0].batch) + b"".join(i.data for i in mixed[1:]) == text + text


# ---- the consumer's side ---------------------------------------------------------------------------------------------------------

class FakeEngine:
    """filter_bgzf_fastq = zlib + fastio.index + a stub (ee of a record is its sequence length); filter_fastq likewise."""

    def __init__(self, hand_back=(), refuse=(), fail=()):
        self.calls, self.fastq_calls = [], []
        self.hand_back, self.refuse, self.fail = set(hand_back), set(refuse), set(fail)

    def _result(self, buf, final, max_records):
        idx, consumed, bad = F.index(buf, final, max_records)
        return types.SimpleNamespace(idx=idx, consumed=consumed, bad=bad, ee=idx[:, F.SEQ_LEN].astype(np.float64),
                                     has_n=np.zeros(len(idx), bool), text=np.frombuffer(buf, np.uint8))

    def filter_bgzf_fastq(self, data, offs, sizes, out_offs, carry=b"", final=True, max_records=None, **kw):
        k = len(self.calls)
        self.calls.append((len(offs), len(carry), bool(final), max_records, kw))
        if k in self.hand_back:
            raise E.MembersNotTaken(0, np.zeros(len(offs), np.uint8), np.full(len(offs), 13, np.uint8))
        if k in self.refuse:
            raise E.NotTaken(1)
        if k in self.fail:
            raise ValueError("Qualities must have positive values.")
        return self._result(bytes(carry) + gzip.decompress(data.tobytes()), final, max_records)

    def filter_fastq(self, buf, final=True, max_records=None, **kw):
        self.fastq_calls.append((len(buf), bool(final), max_records))
        return self._result(bytes(buf), final, max_records)


def drive(text, member_size, batch_text, max_records=1000, engine=None, said=None, blob=None):
    """The text as members of member_size bytes, read in batches of about batch_text bytes of text, through the consumer ->
    (the chunks, the exception it ended with or None, the engine, what was said)."""
    engine = engine or FakeEngine()
    said = [] if said is None else said
    ix = cli._DeviceIndexer(engine, dict(fastq_offset=33, max_len=0), max_records, cli._SaidOnce(said.append, "refused: %s"),
                            members_refused=cli._SaidOnce(said.append, "members: %s"))
    blob = b"".join(M.cut(text, member_size)) if blob is None else blob
    got, err = [], None
    try:
        for item in cli._read_members(reader(blob, threads=4), batch_text):
            for chunk in (ix.take_members(item) if isinstance(item, cli._DeferredMembers) else ix.take(item)):
                got.append(chunk)
    except (F.RecordError, OSError) as e:
        err = e
    return got, err, engine, said


def headers(got):
    return [F.header_of(buf, r) for buf, idx, aux, filtered in got for r in idx]


def expect(text, max_records=1000):
    out, err = [], None
    try:
        for buf, idx in F.FastqChunks(io.BytesIO(text), max_records):
            out += [F.header_of(buf, r) for r in idx]
    except F.RecordError as e:
        err = e
    return out, err


def record_ends(text):
    idx, _, _ = F.index(text, True, 10000)
    return [int(r[F.QUAL_OFF] + r[F.QUAL_LEN]) + 1 for r in idx]


def test_chunks_equal_fastqchunks_wherever_the_member_ends_fall():
    text = b"".join(X.records(40, 71, lo=10, hi=60))
    want, _ = expect(text)
    assert len(want) == 40
    ends = record_ends(text)
    # members of ends[9] bytes end exactly on a record end at least once; 7 and 53 bytes: mid-line and mid-record
    for member_size, batch_text in ((7, 100), (53, 400), (ends[9], ends[9]), (ends[9], 1 << 20), (1 << 15, 1 << 20)):
        got, err, eng, said = drive(text, member_size, batch_text)
        assert err is None and headers(got) == want and said == [], (member_size, batch_text)
        assert all(filtered is not None and aux is None and len(filtered[0]) == len(idx) for buf, idx, aux, filtered in got)
        assert eng.fastq_calls == [] and [c[2] for c in eng.calls] == [False] * (len(eng.calls) - 1) + [True]
        for buf, idx, aux, (ee, has_n) in got:
            assert ee.tolist() == idx[:, F.SEQ_LEN].tolist()
    got, err, eng, said = drive(text, ends[9], ends[9])
    assert eng.calls[1][1] == 0 and len(eng.calls) >= 3      # the first batch ended on a record end: nothing was carried
    got, err, eng, said = drive(text, 53, 400)
    assert any(c[1] > 0 for c in eng.calls)                  # ... and here partial records were
    # the file's last byte without a newline
    got, err, eng, said = drive(text[:-1], 53, 400)
    assert err is None and headers(got) == want and eng.calls[-1][2] is True


def test_a_handed_back_batch_goes_through_inflate_batch_and_filter_fastq_and_is_said_once():
    text = b"".join(X.records(40, 72, lo=10, hi=60))
    got, err, eng, said = drive(text, 53, 400, engine=FakeEngine(hand_back={1, 3}))
    assert err is None and headers(got) == expect(text)[0]
    assert said == ["members: member 0: crc"]
    assert len(eng.fastq_calls) >= 2 and all(filtered is not None for _, _, _, filtered in got)
    # the index's refusal, and a ValueError: fastio.index, and chunks without results for the caller to filter
    got, err, eng, said = drive(text, 53, 400, engine=FakeEngine(refuse={1}, fail={2}))
    assert err is None and headers(got) == expect(text)[0] and said == ["refused: non-ASCII byte"] and eng.fastq_calls == []
    flags = [filtered is None for _, _, _, filtered in got]
    assert True in flags and False in flags


def test_a_corrupt_member_raises_the_host_decoders_error_after_the_chunks_before_it():
    text = b"".join(X.records(40, 73, lo=10, hi=60))
    members = M.cut(text, 300)
    wrong = [m for name, m, why in I.crafted_invalid() if name == "wrong_crc"][0]
    blob = b"".join(members[:5]) + wrong + b"".join(members[5:])
    with pytest.raises(OSError) as plain:
        read_all(reader(blob, threads=4))

    class Checking(FakeEngine):
        def filter_bgzf_fastq(self, data, *a, **kw):
            try:
                gzip.decompress(data.tobytes())
            except Exception:
                self.calls.append(None)
                raise E.MembersNotTaken(0, np.zeros(1, np.uint8), np.full(1, 13, np.uint8))
            return FakeEngine.filter_bgzf_fastq(self, data, *a, **kw)
    got, err, eng, said = drive(text, 0, 1 << 20, engine=Checking(), blob=blob)
    assert isinstance(err, OSError) and str(err) == str(plain.value) and "BGZF block 5" in str(err)
    assert said == ["members: member 0: crc"]


def test_the_record_error_comes_after_the_good_records():
    good = X.records(9, 74)
    text = b"".join(good[:6]) + X.BAD["mismatch"] + b"".join(good[6:])
    for member_size, batch_text in ((13, 50), (100, 100), (1 << 15, 1 << 20)):
        got, err, _, _ = drive(text, member_size, batch_text)
        want, want_err = expect(text)
        assert headers(got) == want and len(want) == 6
        assert err is not None and (err.kind, err.header) == (want_err.kind, want_err.header) == (F.REC_LENGTH_MISMATCH, "bad")


def test_max_records_cuts_a_call_and_the_rest_goes_through_filter_fastq():
    text = b"".join(X.records(25, 75))
    got, err, eng, said = drive(text, 1 << 15, 1 << 20, max_records=10)
    assert err is None and [len(idx) for _, idx, _, _ in got] == [10, 10, 5] and headers(got) == expect(text, 10)[0]
    assert len(eng.calls) == 1 and len(eng.fastq_calls) == 2 and said == []
    assert eng.fastq_calls[0][0] == len(text) - got[0][1][-1][F.QUAL_OFF] - got[0][1][-1][F.QUAL_LEN] - 1
