"""What of the device FASTQ indexer needs no device: the argument checks of mpb_fastq_index_host / mpb_filter_fastq_host (made
before the context is looked at), the CLI's --device_index switch and its eligibility sentence, and the consumer's side of the
switch (cli._DeviceIndexer: deferred blocks, the carried partial record, a handed-back block going through the host, a record
error raised after the good records) against a fake engine whose filter_fastq is fastio.index + a stub.  The lane code on the
host: tests/test_fastq_index_lane_model.py; the kernels: tests/test_gpu_fastq_index.py."""
import ctypes as C
import io
import os
import types

import numpy as np
import pytest

from helpers import fastq_index_texts as X
from moira_amd import _lib as L
from moira_amd import cli
from moira_amd import engine as E
from moira_amd import fastio as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


# ---- the C ABI's argument checks ---------------------------------------------------------------------------------------------

def index_call(text=b"@r\nAC\n+\nII\n", text_bytes=None, final=1, max_records=10, max_len=0, cap=11, null=()):
    lib = L.load()
    idx = np.zeros((max(cap, 1), 6), np.int64)
    n, consumed, bad, why = C.c_int64(-7), C.c_int64(-7), C.c_int32(-7), C.c_int32(-7)
    ptr = lambda name, v: None if name in null else v
    rc = lib.mpb_fastq_index_host(None, ptr("text", text), len(text) if text_bytes is None else text_bytes, final, max_records, max_len,
                                  ptr("idx", idx.ctypes.data), cap, ptr("n", C.byref(n)), ptr("consumed", C.byref(consumed)),
                                  ptr("bad", C.byref(bad)), ptr("why", C.byref(why)))
    return rc, lib.mpb_last_error().decode()


def test_the_entries_and_their_constants_are_declared():
    hdr = open(os.path.join(ROOT, "include", "moira_pb.h")).read()
    for k, name in enumerate(("TAKEN", "NON_ASCII", "LONE_CR", "LINE_TABLE", "ROW_CHECK")):
        assert "#define MPB_FQ_WHY_%s" % name in hdr and len(L.FQ_WHY) == 5
    assert "mpb_fastq_index_host" in L.PROTOTYPES and "mpb_filter_fastq_host" in L.PROTOTYPES
    assert sorted(L.INDEX_KERNEL_NAMES) == [18, 19, 20, 21] and "#define MPB_K_COUNT     22" in hdr
    assert str(E.NotTaken(2)) == "lone carriage return" and E.NotTaken(1).why == 1


def test_index_argument_errors_are_invalid_with_or_without_a_device():
    rc, msg = index_call()
    assert rc == L.E_INVALID and "ctx is NULL" in msg                          # good arguments: only the context is missing
    for kw in (dict(null=("text",)), dict(text_bytes=-1), dict(max_records=-1), dict(max_len=-1), dict(cap=0), dict(null=("idx",)),
               dict(null=("n",)), dict(null=("consumed",)), dict(null=("bad",)), dict(null=("why",))):
        rc, msg = index_call(**kw)
        assert rc == L.E_INVALID and "mpb_fastq_index_host: bad arguments" in msg, kw
    rc, msg = index_call(text_bytes=(1 << 30) + 1)
    assert rc == L.E_INVALID and "at most 1073741824 bytes (1 GiB) of text" in msg
    rc, msg = index_call(text=b"", null=("text",))                              # an empty text needs no pointer
    assert rc == L.E_INVALID and "ctx is NULL" in msg


def test_filter_argument_errors_are_invalid_with_or_without_a_device():
    lib = L.load()
    text = b"@r\nAC\n+\nII\n"
    idx = np.zeros((4, 6), np.int64)
    ee, ns, ps = np.zeros(4), np.zeros(4, np.int32), np.zeros(4, np.uint8)
    n, consumed, bad, why, badrec = C.c_int64(), C.c_int64(), C.c_int32(), C.c_int32(), C.c_int64(5)

    def call(params=E.Engine.params(), offset=33, cap=4, ee_ptr=ee.ctypes.data, text_bytes=len(text)):
        rc = lib.mpb_filter_fastq_host(None, text, text_bytes, 1, 3, 0, idx.ctypes.data, cap, C.byref(n), C.byref(consumed), C.byref(bad),
                                       C.byref(why), offset, 0, C.byref(params) if params is not None else None, 0, ee_ptr,
                                       ns.ctypes.data, ps.ctypes.data, None, None, None, C.byref(badrec))
        return rc, lib.mpb_last_error().decode()
    rc, msg = call()
    assert rc == L.E_INVALID and "ctx is NULL" in msg and badrec.value == -1
    assert "params is NULL" in call(params=None)[1]
    assert "Alpha must be between 0 and 1" in call(params=L.FilterParams(2.0, 0.01, float("nan"), 0, 0))[1]
    assert "fastq_offset 256" in call(offset=256)[1] and "fastq_offset -1" in call(offset=-1)[1]
    assert "mpb_filter_fastq_host: bad arguments" in call(cap=0)[1]
    assert "NULL host buffer" in call(ee_ptr=None)[1]
    assert "1 GiB" in call(text_bytes=(1 << 30) + 1)[1]
    assert all(call(**kw)[0] == L.E_INVALID for kw in (dict(params=None), dict(offset=256), dict(cap=0), dict(ee_ptr=None)))


# ---- the switch and its sentence ---------------------------------------------------------------------------------------------------

def test_the_parser_knows_the_switch_and_it_is_off_by_default():
    p = cli.build_parser()
    assert p.parse_args(["-ffq", "x"]).device_index is False
    assert p.parse_args(["-ffq", "x", "--device_index"]).device_index is True
    text = " ".join(p.format_help().split())
    assert "--device_index" in text and "Paired input and fasta+qual input stay on the host indexer" in text


def test_it_is_one_more_row_and_one_more_attribute():
    assert [r[0] for r in cli._DEVICE_PATHS] == ["device_pack", "device_contigs", "device_index", "device_compress", "device_inflate"]
    assert cli._DevicePaths().index is False and cli._DevicePaths(("device_pack",)).index is False
    said = []
    d = cli._DevicePaths({"device_pack", "device_index"}, 0, said.append)
    assert d.index and d.pack and d.engine is None                             # (no auxiliary engine: the filter's own context indexes)
    d.index_refused(E.NotTaken(2)), d.index_refused(E.NotTaken(1))
    assert said == ["--device_index: the device did not take a block (lone carriage return): the host indexer is used for it."]


def fake_backend(paired_text=True, with_index=True):
    be = lambda *a, **k: None
    be.matrix = lambda *a, **k: None
    be.methods = ("poisson_binomial", "poisson")
    be.engine = types.SimpleNamespace(device=0)
    if with_index:
        be.engine.filter_fastq = lambda *a, **k: None
    if paired_text:
        be.text = lambda *a, **k: None
        be.text_choice = lambda *a, **k: {}
    return be


def test_eligibility():
    from test_cli_golden import reference_args
    fq = os.path.join(GOLD, "test1.fastq.gz")
    single = reference_args(paired=False, forward_fastq=fq)
    assert cli._device_index_eligible(single, fake_backend())
    assert not cli._device_index_eligible(single, fake_backend(paired_text=False))          # several GPUs: no text entry
    assert not cli._device_index_eligible(single, fake_backend(with_index=False))
    assert not cli._device_index_eligible(reference_args(paired=True, forward_fastq=fq, reverse_fastq=fq), fake_backend())
    assert not cli._device_index_eligible(reference_args(paired=False, forward_fasta="a", forward_qual="b"), fake_backend())
    assert not cli._device_index_eligible(reference_args(paired=False, forward_fastq=fq, fastq_offset=300), fake_backend())


def test_the_switch_without_a_gpu_or_without_device_pack_says_so_once_and_changes_no_file(tmp_path, oracle):
    from test_cli_golden import oracle_backend, reference_args
    fq = os.path.join(GOLD, "test1.fastq.gz")
    files = {}
    for name, kw in (("off", {}), ("on", dict(device_index=True)), ("both", dict(device_index=True, device_pack=True)),
                     ("quiet", dict(device_index=True, nowarnings=True))):
        log = io.StringIO()
        a = reference_args(paired=False, forward_fastq=fq, output_prefix=str(tmp_path / name), **kw)
        assert cli.main(a, backend=oracle_backend(oracle), out=log) == 0
        files[name] = {p.split(".", 1)[1]: open(os.path.join(str(tmp_path), p), "rb").read()
                       for p in sorted(os.listdir(str(tmp_path))) if p.startswith(name + ".")}
        lines = [l for l in log.getvalue().splitlines() if "does not apply to this run" in l]
        want = {"off": [], "on": ["--device_index"], "both": ["--device_pack", "--device_index"], "quiet": []}[name]
        assert [l.split(" ")[0] for l in lines] == want
        if "--device_index" in want:
            assert lines[-1].endswith("with --device_pack): the host indexer is used.")
    assert len(files["off"]) >= 3 and files["on"] == files["off"] == files["both"] == files["quiet"]


# ---- the consumer's side ---------------------------------------------------------------------------------------------------------

class FakeEngine:
    """filter_fastq = fastio.index + a stub: ee of a record is its sequence length, has_n whether it holds an 'N'."""

    def __init__(self, refuse=(), fail=()):
        self.calls, self.refuse, self.fail = [], set(refuse), set(fail)

    def filter_fastq(self, buf, final=True, max_records=None, **kw):
        k = len(self.calls)
        self.calls.append((len(buf), bool(final), max_records, kw))
        if k in self.refuse:
            raise E.NotTaken(2)
        if k in self.fail:
            raise ValueError("Qualities must have positive values.")
        idx, consumed, bad = F.index(buf, final, max_records)
        ee = idx[:, F.SEQ_LEN].astype(np.float64)
        has_n = np.array([b"N" in bytes(buf[r[F.SEQ_OFF]:r[F.SEQ_OFF] + r[F.SEQ_LEN]]) for r in idx], bool)
        return types.SimpleNamespace(idx=idx, consumed=consumed, bad=bad, ee=ee, has_n=has_n)


def blocks_of(text, size):
    return [cli._DeferredBlock(text[a:a + size], False) for a in range(0, len(text), size)] + [cli._DeferredBlock(b"", True)]


def drive(text, size, max_records=1000, engine=None, said=None):
    """-> (the chunks the indexer yields, the exception it ended with or None, the engine)."""
    engine = engine or FakeEngine()
    refused = cli._SaidOnce((said if said is not None else []).append, "refused: %s")
    ix = cli._DeviceIndexer(engine, dict(fastq_offset=33, max_len=0), max_records, refused)
    got, err = [], None
    try:
        for b in blocks_of(text, size):
            for chunk in ix.take(b):                         # (taken one by one, as the run does: what came before an error counts)
                got.append(chunk)
    except F.RecordError as e:
        err = e
    return got, err, engine


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


def test_read_blocks_end_with_an_empty_final_block():
    got = list(cli._read_blocks(io.BytesIO(b"abcdefg"), 3))
    assert [(b.data, b.eof) for b in got] == [(b"abc", False), (b"def", False), (b"g", False), (b"", True)]
    assert [(b.data, b.eof) for b in cli._read_blocks(io.BytesIO(b""), 3)] == [(b"", True)]


@pytest.mark.parametrize("size", [7, 50, 333, 1 << 20])
def test_partial_records_are_carried_from_block_to_block(size):
    text = b"".join(X.records(40, 31))
    got, err, eng = drive(text, size)
    want, _ = expect(text)
    assert err is None and headers(got) == want and len(want) == 40
    assert all(filtered is not None and aux is None and len(filtered[0]) == len(idx) for buf, idx, aux, filtered in got)
    assert not any(c[1] for c in eng.calls[:-1])             # no call but the last may be final ...
    open_got, err, open_eng = drive(text[:-1], size)         # ... and it is when the text ends without a newline
    assert err is None and headers(open_got) == want and open_eng.calls[-1][1] is True
    if size == 7:
        assert len(eng.calls) > 3 * 40                       # (every record is carried across many blocks)
    for buf, idx, aux, (ee, has_n) in got:
        assert ee.tolist() == idx[:, F.SEQ_LEN].tolist()


def test_a_block_with_more_records_than_a_chunk_holds_gives_several_chunks():
    text = b"".join(X.records(25, 32))
    got, err, eng = drive(text, 1 << 20, max_records=10)
    assert err is None and [len(idx) for _, idx, _, _ in got] == [10, 10, 5] and headers(got) == expect(text, 10)[0]


def test_trailing_lines_that_make_no_record_are_dropped_at_the_end():
    text = b"".join(X.records(5, 33)) + b"@x\nAC\n+\n"
    for size in (11, 1 << 20):
        got, err, _ = drive(text, size)
        assert err is None and len(headers(got)) == 5


def test_the_record_error_comes_after_the_good_records():
    good = X.records(9, 34)
    text = b"".join(good[:6]) + X.BAD["mismatch"] + b"".join(good[6:])
    for size in (13, 100, 1 << 20):
        got, err, _ = drive(text, size)
        want, want_err = expect(text)
        assert headers(got) == want and len(want) == 6
        assert err is not None and (err.kind, err.header) == (want_err.kind, want_err.header) == (F.REC_LENGTH_MISMATCH, "bad")


def test_a_handed_back_block_goes_through_the_host_and_is_said_once():
    text = b"".join(X.records(30, 35))
    said = []
    got, err, eng = drive(text, 400, engine=FakeEngine(refuse={1, 3}, fail={2}), said=said)
    assert err is None and headers(got) == expect(text)[0]
    assert said == ["refused: lone carriage return"]
    flags = [filtered is None for _, idx, _, filtered in got]
    assert True in flags and False in flags                  # the host's chunks come without results: the caller filters them


def test_what_the_host_calls_unsupported_is_the_runs_to_take():
    text = b"".join(X.records(3, 36)) + X.rec(b"x", b"A\rC", b"III")
    ix = cli._DeviceIndexer(FakeEngine(refuse={0}), {}, 100, lambda e: None)
    with pytest.raises(F.Unsupported):
        list(ix.take(cli._DeferredBlock(text, True)))


# ---- the capacity loop of the text-alone entries (engine._ask_again) against a scripted call -----------------------------------------

def scripted(answers):
    """-> (call, the (cap, out_cap) pairs it was asked with): the k-th call answers answers[k] = (rc, rows needed, bytes needed)."""
    asked = []

    def call(cap, out_cap):
        asked.append((cap, out_cap))
        return answers[len(asked) - 1]
    return call, asked


def test_a_guess_that_is_enough_is_one_call():
    call, asked = scripted([(L.OK, 8, None)])
    assert E._ask_again(call, 11, 1 << 62) == (L.OK, 1) and asked == [(11, None)]
    call, asked = scripted([(L.E_INVALID, 8, None)])                     # refused for another reason: not asked again
    assert E._ask_again(call, 11, 1 << 62) == (L.E_INVALID, 1) and asked == [(11, None)]


def test_a_guess_too_small_is_asked_once_more_with_the_rows_needed():
    call, asked = scripted([(L.E_INVALID, 41, None), (L.OK, 41, None)])
    assert E._ask_again(call, 11, 1 << 62) == (L.OK, 2) and asked == [(11, None), (41, None)]
    # through Engine._fastq_call (it needs no context): the guess is 64 bytes a record, the second call has n + 1 rows
    text, seen = b"@r\nAC\n+\nII\n" * 500, []

    def entry(addr, nbytes, final, limit, max_len, idx_ptr, cap, n, consumed, bad, why):
        seen.append((cap, limit))
        n._obj.value = 500
        return L.E_INVALID if cap < 501 else L.OK
    rc, idx, n, consumed, bad, why = E.Engine._fastq_call(None, text, True, None, 0, entry)
    assert seen == [(len(text) // 64 + 65, 1 << 62), (501, 1 << 62)] and (rc, len(idx), n) == (L.OK, 501, 500)


def test_at_the_record_limit_the_error_surfaces_without_a_second_call():
    call, asked = scripted([(L.E_INVALID, 30, None)])
    rc, calls = E._ask_again(call, 11, 10)                              # cap == limit + 1: more rows cannot be the reason
    assert (rc, calls) == (L.E_INVALID, 1) and asked == [(11, None)]
    with pytest.raises(ValueError):
        L.check(rc)
    with pytest.raises(ValueError, match="max_records must not be negative"):
        E._record_limit(-1)
    assert E._record_limit(None) == 1 << 62 and E._record_limit(7) == 7


def test_the_paired_entrys_two_capacities_grow_as_they_did():
    # rows too small, then bytes too small: + 16 bytes per missing row, then n_pairs * rec_cap
    call, asked = scripted([(L.E_INVALID, 25, 0), (L.E_INVALID, 25, 5000), (L.OK, 25, 5000)])
    assert E._ask_again(call, 10, 1 << 62, 1000, grow_out=True) == (L.OK, 3)
    assert asked == [(10, 1000), (25, 1000 + 16 * 15), (25, 5000)]
    # a byte capacity the caller gave is not grown by the rows step
    call, asked = scripted([(L.E_INVALID, 25, 0), (L.OK, 25, 900)])
    assert E._ask_again(call, 10, 1 << 62, 1000, grow_out=False) == (L.OK, 2) and asked == [(10, 1000), (25, 1000)]
    # enough bytes, another reason: the error surfaces
    call, asked = scripted([(L.E_INVALID, 10, 1000)])
    assert E._ask_again(call, 10, 1 << 62, 1000, grow_out=True) == (L.E_INVALID, 1)


def test_a_handed_back_bgzf_member_is_not_asked_again():
    """Engine.filter_bgzf_fastq reports no rows to ask for once a member was handed back (first >= 0), whatever n says."""
    call, asked = scripted([(L.E_INVALID, 0, None)])
    assert E._ask_again(call, 11, 1 << 62) == (L.E_INVALID, 1) and asked == [(11, None)]
    # the method itself over a scripted entry: n says 999 rows, far above the guess, but member 0 was handed back
    caps = []

    def entry(*a):
        first, cap, n = a[16], a[19], a[20]
        caps.append(cap)
        first._obj.value, n._obj.value = 0, 999
        return L.E_INVALID
    fake = types.SimpleNamespace(ctx=None, lib=types.SimpleNamespace(mpb_filter_bgzf_fastq_host=entry), params=E.Engine.params)
    with pytest.raises(ValueError):
        E.Engine.filter_bgzf_fastq(fake, b"\0" * 64, [0], [64], [0, 100])
    assert caps == [100 // 64 + 65]
