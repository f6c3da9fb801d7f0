"""The FASTQ record index on the GPU (include/moira_pb.h: mpb_fastq_index_host, mpb_filter_fastq_host; Engine.fastq_index,
Engine.filter_fastq; the CLI's --device_index).  fastio.index (mio_fastq_index) is the reference everywhere: all six columns,
consumed and the bad record are compared with array_equal, and "device, else host" must equal the host alone.  filter_fastq is
compared bit for bit (ee as uint64, NaN included) with fastio.index + Engine.filter_text.  The directed texts are
tests/helpers/fastq_index_texts.py's; the same texts go through the lane code on the host in
tests/test_fastq_index_lane_model.py."""
import gzip
import os

import numpy as np
import pytest

from helpers import fastq_index_texts as X
from moira_amd import cli
from moira_amd import engine as E
from moira_amd import fastio as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def golden_text():
    return gzip.open(os.path.join(GOLD, "test1.fastq.gz"), "rb").read()


def host_index(text, final, max_records):
    """fastio.index with a row count the text can bear -> (idx, consumed, (kind, header, row) or None), or None: unsupported."""
    cap = min(max_records, len(text) // 4 + 1)
    try:
        idx, consumed, bad = F.index(text, bool(final), cap)
    except F.Unsupported:
        return None
    if bad is None:
        return idx, consumed, None
    # the row after the last good one is the offender's: index once more into an array of our own to look at it
    import ctypes as C
    full = np.zeros((cap + 1, 6), np.int64)
    c, b = C.c_int64(0), C.c_int32(0)
    n = F.load().mio_fastq_index(text, len(text), 1 if final else 0, cap, full.ctypes.data, C.addressof(c), C.addressof(b))
    assert n == len(idx) and b.value == bad.kind
    return idx, consumed, (bad.kind, bad.header, full[n].tolist())


def same_as_host(eng, name, text, final, max_records):
    want = host_index(text, final, max_records)
    assert want is not None, name
    idx, consumed, bad = eng.fastq_index(text, final=bool(final), max_records=None if max_records == X.BIG else max_records)
    assert idx.dtype == np.int64 and idx.shape == want[0].shape and np.array_equal(idx, want[0]), name
    assert consumed == want[1], name
    assert (bad is None) == (want[2] is None), name
    if bad is not None:
        assert (bad.kind, bad.header, bad.row.tolist()) == want[2], name


# ---- the directed texts ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("group", ["placement", "endings", "limits", "bad_records", "headers", "not_looked_at"])
def test_directed_texts_equal_the_host_index(eng, group):
    cases = getattr(X, group)()
    assert len(cases) >= 2
    for name, text, final, max_records in cases:
        same_as_host(eng, name, text, final, max_records)


def test_the_row_after_the_last_good_one_is_the_offenders(eng):
    good = X.records(4, 41)
    text = b"".join(good[:3]) + X.rec(b"@the:bad one", b"ACG", b"II") + good[3]
    idx, consumed, bad = eng.fastq_index(text)
    assert len(idx) == 3 and consumed == len(b"".join(good[:3]))
    assert bad.kind == F.REC_LENGTH_MISMATCH and bad.header == "the_bad" and bad.row[F.SEQ_LEN] == 3 and bad.row[F.QUAL_LEN] == 2
    assert text[bad.row[F.SEQ_OFF]:bad.row[F.SEQ_OFF] + 3] == b"ACG"


def test_handed_back_with_the_right_reason_and_device_else_host_is_the_host(eng):
    for name, text, final, max_records, why in X.handed_back():
        with pytest.raises(E.NotTaken) as e:
            eng.fastq_index(text, final=bool(final), max_records=None if max_records == X.BIG else max_records)
        assert e.value.why == why, name
        with pytest.raises(E.NotTaken) as e:
            eng.filter_fastq(text, final=bool(final), max_records=None if max_records == X.BIG else max_records)
        assert e.value.why == why, name
    # "device, else host" against the host alone, on texts of both kinds
    for name, text, final, max_records in [c[:4] for c in X.handed_back()] + X.bad_records()[:6]:
        want = host_index(text, final, max_records)
        try:
            idx, consumed, bad = eng.fastq_index(text, final=bool(final), max_records=None if max_records == X.BIG else max_records)
            got = (idx, consumed, None if bad is None else bad.kind)
        except E.NotTaken:
            h = host_index(text, final, max_records)
            got = None if h is None else (h[0], h[1], None if h[2] is None else h[2][0])
        if want is None:
            assert got is None, name
        else:
            assert np.array_equal(got[0], want[0]) and got[1] == want[1] and got[2] == (None if want[2] is None else want[2][0]), name


def test_argument_errors(eng):
    with pytest.raises(ValueError, match="max_records must not be negative"):
        eng.fastq_index(b"@r\nA\n+\nI\n", max_records=-1)
    import ctypes as C
    text = b"".join(X.records(5, 42))
    idx = np.zeros((3, 6), np.int64)
    n, consumed, bad, why = C.c_int64(0), C.c_int64(0), C.c_int32(0), C.c_int32(0)
    rc = eng.lib.mpb_fastq_index_host(eng.ctx, text, len(text), 1, 100, 0, idx.ctypes.data, 3, C.byref(n), C.byref(consumed),
                                      C.byref(bad), C.byref(why))
    assert rc == -1 and b"idx_cap_rows 3 is too small: the text holds 5 records" in eng.lib.mpb_last_error() and n.value == 5
    # ... which is what lets a caller who guessed ask again: 3,000 records of 13 bytes against a guess of 64 bytes each
    many = b"@\nA\n+\nI\n" * 3000
    got = eng.fastq_index(many)
    assert len(got[0]) == 3000 and got[1] == len(many) and np.array_equal(got[0], host_index(many, 1, X.BIG)[0])


# ---- larger inputs ---------------------------------------------------------------------------------------------------------------

def test_more_tiles_than_one_scan_trip_holds(eng):
    """1,030 tiles of 16 KiB (a scan trip holds 1,024): identical short records, and no newline count that is a multiple of a tile's."""
    one = X.rec(b"r", b"ACGTACGTACG", b"IIIIIIIIIII")
    n = (1030 * X.T) // len(one) + 1
    text = one * n
    assert len(text) > 1030 * X.T
    idx, consumed, bad = eng.fastq_index(text)
    assert bad is None and consumed == len(text) and len(idx) == n
    want = np.array([1, 1, 3, 11, 17, 11], np.int64)[None, :] + np.array([1, 0, 1, 0, 1, 0], np.int64)[None, :] * (np.arange(n, dtype=np.int64) * len(one))[:, None]
    assert np.array_equal(idx, want)
    cut = text[:1027 * X.T + 5]                              # ... and cut inside a record behind the trip's end, not final
    idx, consumed, bad = eng.fastq_index(cut, final=False)
    assert len(idx) == len(cut) // len(one) and consumed == len(idx) * len(one) and np.array_equal(idx, want[:len(idx)])


def test_golden_reads_whole_and_cut(eng, golden_text):
    same_as_host(eng, "golden", golden_text, 1, X.BIG)
    assert len(eng.fastq_index(golden_text)[0]) == 1000
    rng = np.random.default_rng(50)
    for at in rng.integers(0, len(golden_text) + 1, 50).tolist():
        same_as_host(eng, "golden cut at %d" % at, golden_text[:at], 0, X.BIG)


def test_every_fuzz_text_is_taken_and_equals_the_host(eng):
    cases = X.fuzz()
    assert len(cases) == 2000
    for name, text, final, max_records in cases:
        same_as_host(eng, name, text, final, max_records)    # (a NotTaken would fail the test: zero handed back)


# ---- filter_fastq against fastio.index + Engine.filter_text -------------------------------------------------------------------------

def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same_filter(eng, text, final=True, max_records=None, **kw):
    idx, consumed, bad = F.index(text, final, len(text) // 4 + 1 if max_records is None else max_records)
    want = eng.filter_text(text, idx, **kw)
    got = eng.filter_fastq(text, final=final, max_records=max_records, **kw)
    assert np.array_equal(got.idx, idx) and got.consumed == consumed
    assert (got.bad is None) == (bad is None) and (bad is None or (got.bad.kind, got.bad.header) == (bad.kind, bad.header))
    assert np.array_equal(bits(got.ee), bits(want.ee)) and np.array_equal(got.ns, want.ns) and np.array_equal(got.passed, want.passed)
    assert np.array_equal(got.lens, want.lens) and np.array_equal(got.has_n, want.has_n)
    assert (got.n_pass, got.n_fail, got.n_overflow) == (want.n_pass, want.n_fail, want.n_overflow)
    return got


def test_filter_fastq_on_the_golden_reads(eng, golden_text):
    got = same_filter(eng, golden_text)
    assert len(got.ee) == 1000 and 0 < got.n_pass < 1000
    same_filter(eng, golden_text, max_len=100)
    same_filter(eng, golden_text, lower_n_is_base=True)
    same_filter(eng, golden_text, poisson=True)
    same_filter(eng, golden_text, poisson=True, poisson_device_tail=True)
    same_filter(eng, golden_text[:len(golden_text) // 2], final=False)
    same_filter(eng, golden_text, max_records=300)
    same_filter(eng, b"")


def test_filter_fastq_in_three_pieces(eng, golden_text, monkeypatch):
    idx, _, _ = F.index(golden_text, True, 2000)
    stride = (int(idx[:, F.QUAL_LEN].max()) + 127) // 128 * 128
    monkeypatch.setenv("MPB_TEXT_PIECE_BYTES", str(400 * stride))               # 1,000 rows in pieces of 400: three pieces
    same_filter(eng, golden_text)
    same_filter(eng, golden_text, poisson=True)


def test_filter_fastq_with_a_bad_record_behind_100_good_ones(eng):
    good = X.records(120, 43, lo=20, hi=150)
    text = b"".join(good[:100]) + X.rec(b"bad", b"A" * 400, b"I" * 399) + b"".join(good[100:])
    got = same_filter(eng, text)
    assert len(got.ee) == 100 and got.bad.kind == F.REC_LENGTH_MISMATCH and got.bad.header == "bad"
    assert int(got.lens.max()) <= 150                        # the offender's 399 bases did not widen the matrix


def test_a_quality_out_of_range_is_the_same_valueerror(eng):
    good = X.records(30, 44)
    text = b"".join(good[:17]) + X.rec(b"x", b"ACG", b"I I") + b"".join(good[17:])           # a blank is below offset 33
    idx, _, _ = F.index(text, True, 100)
    with pytest.raises(ValueError) as want:
        eng.filter_text(text, idx)
    with pytest.raises(ValueError) as got:
        eng.filter_fastq(text)
    assert str(got.value) == str(want.value) == "Qualities must have positive values."
    assert got.value.bad_record == want.value.bad_record == 17
    # (a quality above 254 needs a byte >= 0x80 at offset 0: such a text is handed back, and the host path says it)
    with pytest.raises(E.NotTaken):
        eng.filter_fastq(b"".join(good) + X.rec(b"x", b"AC", b"\xff\xff"), fastq_offset=0, poisson=True)


def test_the_kernels_show_in_the_timing_table(eng):
    eng.timing(True)
    eng.timing_reset()
    eng.fastq_index(b"".join(X.records(10, 45)))
    t = eng.kernel_times()
    eng.timing(False)
    assert all(t[k][1] == 1 for k in ("fq_lines", "fq_scan", "fq_starts", "fq_rows")), t


# ---- the CLI ---------------------------------------------------------------------------------------------------------------------

def watching_backend():
    import threading
    be = cli.make_gpu_backend(None)
    seen = {"fastq": [], "text": [], "threads": set()}
    inner_fastq, inner_text = be.engine.filter_fastq, be.text

    def filter_fastq(buf, **kw):
        seen["threads"].add(threading.get_ident())
        r = inner_fastq(buf, **kw)
        seen["fastq"].append((len(buf), len(r.idx)))         # (blocks the device took: counted once it has returned)
        return r

    def text(*a, **kw):
        seen["threads"].add(threading.get_ident())
        seen["text"].append(len(a[1]))
        return inner_text(*a, **kw)
    be.engine.filter_fastq, be.text = filter_fastq, text
    return be, seen


def run_cli(tmp_path, name, src, index, **kw):
    """-> (the files, the exception or None, what the backend saw)."""
    import io
    from test_cli_golden import reference_args
    a = reference_args(paired=False, forward_fastq=src, output_prefix=str(tmp_path / name), device_pack=True, device_index=index, **kw)
    be, seen = watching_backend()
    log, err = io.StringIO(), None
    try:
        try:
            assert cli.main(a, backend=be, out=log) == 0
        except (cli.EmptySeqError, cli.EmptyQualError, cli.LengthMismatchError) as e:
            err = e
    finally:
        be.engine.close()
    files = {p.split(".", 1)[1]: open(os.path.join(str(tmp_path), p), "rb").read()
             for p in sorted(os.listdir(str(tmp_path))) if p.startswith(name + ".")}
    seen["log"] = log.getvalue()
    return files, err, seen


@pytest.mark.parametrize("kw", [{}, dict(collapse=False), dict(collapse=False, truncate=100), dict(truncate=150)],
                         ids=["default", "no_collapse", "no_collapse_truncate", "truncate"])
def test_cli_golden_run_is_identical_with_the_switch(tmp_path, kw):
    src = os.path.join(GOLD, "test1.fastq.gz")
    off, _, seen_off = run_cli(tmp_path, "off", src, False, **kw)
    on, _, seen_on = run_cli(tmp_path, "on", src, True, **kw)
    assert seen_off["fastq"] == [] and sum(seen_off["text"]) == 1000
    assert sum(n for _, n in seen_on["fastq"]) == 1000 and seen_on["text"] == []          # the device indexed every record
    assert "--device_index" not in seen_on["log"]
    assert off.keys() == on.keys() and len(off) >= 3 and off == on
    if not kw:
        from test_cli_golden import same_files
        same_files(str(tmp_path / "on"), "forward")


def test_cli_carries_partial_records_across_blocks_on_one_thread(tmp_path, monkeypatch, golden_text):
    """Blocks of 50,000 bytes: the golden text in more than three blocks, a partial record carried from each to the next; every
    call on the context comes from the thread that runs cli.main (calls on one context must not overlap)."""
    import threading
    src = str(tmp_path / "plain.fastq")
    with open(src, "wb") as f:
        f.write(golden_text)
    off, _, _ = run_cli(tmp_path, "off", src, False, collapse=False)
    monkeypatch.setattr(cli, "DEVICE_INDEX_BLOCK", 50000)
    on, _, seen = run_cli(tmp_path, "on", src, True, collapse=False)
    # (one call per block that brought text: the text ends with its newline, so the empty last block leaves nothing to index)
    assert len(seen["fastq"]) == len(golden_text) // 50000 + 1 > 4 and sum(n for _, n in seen["fastq"]) == 1000
    assert all(size % 50000 != 0 for size, _ in seen["fastq"][1:-1])            # (a carry came with every block after the first)
    assert seen["threads"] == {threading.get_ident()}
    assert off == on and len(off) >= 3


def test_cli_bad_record_in_the_second_block_ends_the_same_way(tmp_path, monkeypatch, golden_text):
    lines = golden_text.split(b"\n")
    at = 4 * 600 + 3                                         # the quality line of record 600: one character short
    lines[at] = lines[at][:-1]
    src = str(tmp_path / "bad.fastq")
    with open(src, "wb") as f:
        f.write(b"\n".join(lines))
    monkeypatch.setattr(cli, "DEVICE_INDEX_BLOCK", 200000)
    monkeypatch.setattr(cli, "CHUNK_READS", 256)
    assert len(b"\n".join(lines[:at])) > 200000
    off, err_off, _ = run_cli(tmp_path, "off", src, False, collapse=False)
    on, err_on, seen = run_cli(tmp_path, "on", src, True, collapse=False)
    assert isinstance(err_off, cli.LengthMismatchError) and type(err_on) is type(err_off) and str(err_on) == str(err_off)
    assert err_on.args == err_off.args
    assert sum(n for _, n in seen["fastq"]) == 600 and off == on and sum(len(v) for v in on.values()) > 10000


def test_cli_a_block_the_device_hands_back_goes_through_the_host(tmp_path, monkeypatch, golden_text):
    """A byte >= 0x80 in a header behind the first block: that block is indexed on the host, which says unsupported, and the run
    starts over with the line parser -- as it does without the switch."""
    lines = golden_text.split(b"\n")
    lines[4 * 700] += b" caf\xc3\xa9"
    src = str(tmp_path / "latin.fastq")
    with open(src, "wb") as f:
        f.write(b"\n".join(lines))
    monkeypatch.setattr(cli, "DEVICE_INDEX_BLOCK", 200000)
    off, err_off, _ = run_cli(tmp_path, "off", src, False, collapse=False)
    on, err_on, seen = run_cli(tmp_path, "on", src, True, collapse=False)
    assert err_off is None and err_on is None and off == on and len(on) >= 3
    assert seen["log"].count("--device_index: the device did not take a block (non-ASCII byte)") == 1
