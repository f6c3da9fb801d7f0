"""Reads of up to 65535 bases (MPB_MAX_LEN) through every kernel of the device text path on the GPU: the FASTQ index (k_fq_*),
k_pack_text, the fused filter_fastq / filter_text / filter_bgzf_fastq, the formatter (k_fmt_*), collapse (k_col_*) and fasta+qual
(k_fa_*).  The inputs are tests/helpers/long_read_inputs.py's (their preconditions: tests/test_long_read_inputs.py); the references
are the host's -- fastio.index, fastio.pack, the oracle's filter_batch on fastio.pack's matrix, fastio.format_records,
fastio.py2_hashes, fastio.fasta_qual_index -- and every comparison is bit for bit.  What the short-read GPU tests of these
stages never reach: a 16 KiB index tile without a newline, hundreds of steps of a lane group's running-base loop, thousands of
words of cl_hash and cl_equal, packed rows of 65536 bytes, pieces of one row, records that span several BGZF members."""
import numpy as np
import pytest

from helpers import bgzf_fastq_inputs as M
from helpers import collapse_inputs
from helpers import fasta_qual_inputs as FA
from helpers import long_read_inputs as X
from moira_amd import _lib as L
from moira_amd import engine as E
from moira_amd import fastio as F
from test_gpu_fasta_qual import raw_index
from test_gpu_fastq_index import host_index, same_as_host
from test_gpu_format_text import check_compressed
from test_gpu_pack_text import I64_MAX, check_against_mio_pack, run_pack

pytestmark = pytest.mark.gpu

BIG = 1 << 40
STRIDE = 65536
KINDS = (F.FMT_FASTA, F.FMT_QUAL, F.FMT_FASTQ)


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(0)
    yield e
    e.close()


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def oracle_of(oracle, text, idx, fastq_offset=33, max_len=0):
    """The oracle's results on fastio.pack's matrix of the records: (ee bits, ns, passed, lens, has_n)."""
    q, lens, flags = F.pack(text, idx, None, fastq_offset, max_len, stride=STRIDE)
    ee, ns, ps, rows = oracle.filter_batch(q, lens=lens, threads=8)
    assert rows.max() < 16384 and not np.isnan(ee).any()
    return bits(ee), ns, ps.astype(bool), lens, flags.astype(bool)


def same_results(res, want):
    ee, ns, ps, lens, flags = want
    assert np.array_equal(bits(res.ee), ee) and np.array_equal(res.ns, ns) and np.array_equal(res.passed, ps)
    assert np.array_equal(res.lens, lens) and np.array_equal(res.has_n, flags)
    assert res.n_pass == int(ps.sum())


@pytest.fixture(scope="module")
def fastq_want(oracle):
    text, idx = X.fastq_text()
    w = oracle_of(oracle, text, idx)
    assert 0 < w[2].sum() < len(idx) and w[4].sum() == 1
    return w


# ---- the index ----------------------------------------------------------------------------------------------------------------------

def index_cases():
    out = []
    for tag, nl in (("lf", b"\n"), ("crlf", b"\r\n")):
        text, idx = X.fastq_text(nl)
        cut = int(idx[1, F.QUAL_OFF]) + 40000                # inside the 65535-base quality line
        for final in (1, 0):
            out.append(("%s/whole/%d" % (tag, final), text, final, BIG))
            out.append(("%s/cut_in_quality/%d" % (tag, final), text[:cut], final, BIG))
            for m in (1, 2, 3, 4):                           # the cut just before and just behind a long record
                out.append(("%s/max_records%d/%d" % (tag, m, final), text, final, m))
    return out


INDEX_CASES = index_cases()


@pytest.mark.parametrize("case", INDEX_CASES, ids=[c[0] for c in INDEX_CASES])
def test_the_index_of_long_records_is_the_hosts(eng, case):
    name, text, final, max_records = case
    same_as_host(eng, name, text, final, max_records)
    if "cut_in_quality/0" in name:
        assert len(eng.fastq_index(text, final=False)[0]) == 1            # (the long record waits for its end)


@pytest.mark.parametrize("byte,why", [(b"\r", 2), (b"\x80", 1)], ids=["lone_cr", "non_ascii"])
def test_a_byte_the_index_refuses_in_a_tile_without_newline_of_the_open_last_line(eng, byte, why):
    good, idx = X.fastq_text()
    tail = bytearray(b"@open " + b"x" * (3 * X.T))
    at = (len(good) // X.T + 2) * X.T + 100 - len(good)      # inside the second whole tile of the tail
    tail[at:at + 1] = byte
    text = good + bytes(tail)
    tile = text[(len(good) + at) // X.T * X.T:][:X.T]
    assert len(tile) == X.T and b"\n" not in tile and byte in tile
    same_as_host(eng, "open tail, not final", text, 0, BIG)            # behind the last newline of a non-final text: not looked at
    assert len(eng.fastq_index(text, final=False)[0]) == len(idx)
    assert host_index(text, 1, BIG) is None                 # final: the host calls it unsupported, the device hands it back
    for call in (eng.fastq_index, eng.filter_fastq):
        with pytest.raises(E.NotTaken) as e:
            call(text, final=True)
        assert e.value.why == why


# ---- the pack -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("max_len", [0, 40000])
def test_rows_of_65536_bytes_are_mio_packs_matrix(eng, max_len):
    text, idx = X.fastq_text()
    q, lens, flags = check_against_mio_pack(eng, text, idx, stride=STRIDE, max_len=max_len)
    assert q.shape == (len(idx), STRIDE) and lens.max() == (max_len or X.MAX_LEN) and flags.sum() == 1


def test_a_quality_out_of_range_at_base_65534_is_reported_at_its_row(eng):
    text, idx = X.fastq_text()
    b = bytearray(text)
    b[int(idx[1, F.QUAL_OFF]) + 65534] = 32                  # the last base of the longest read: below offset 33
    q, lens, flags, status = run_pack(eng, bytes(b), idx, stride=STRIDE)
    assert status.tolist() == [1, I64_MAX]
    with pytest.raises(ValueError, match="Qualities must have positive values") as e:
        eng.filter_text(bytes(b), idx)
    assert e.value.bad_record == 1


# ---- the filter ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("piece", [None, 3 * STRIDE, 1000], ids=["one_piece", "three_rows", "less_than_a_row"])
def test_the_fused_and_the_indexed_filter_equal_the_oracle(eng, fastq_want, monkeypatch, piece):
    """MPB_TEXT_PIECE_BYTES of three rows: eleven pieces; of less than one row: text_piece_rows clamps to one row a piece."""
    text, idx = X.fastq_text()
    if piece is not None:
        monkeypatch.setenv("MPB_TEXT_PIECE_BYTES", str(piece))
    got = eng.filter_fastq(text)
    assert np.array_equal(got.idx, idx) and got.consumed == len(text) and got.bad is None
    same_results(got, fastq_want)
    same_results(eng.filter_text(text, idx), fastq_want)


def test_the_filter_with_crlf_and_truncated_rows_equals_the_oracle(eng, oracle):
    text, idx = X.fastq_text(b"\r\n")
    want = oracle_of(oracle, text, idx, max_len=40000)
    got = eng.filter_fastq(text, max_len=40000)
    assert np.array_equal(got.idx, idx)
    same_results(got, want)
    same_results(eng.filter_text(text, idx, max_len=40000), want)


# ---- members -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("carry", [0, 40000], ids=["no_carry", "carry_ends_in_a_long_line"])
def test_records_that_span_five_members_equal_filter_fastq_on_the_text(eng, fastq_want, carry):
    text, idx = X.fastq_text()
    assert int(idx[1, F.SEQ_OFF]) < carry < int(idx[1, F.SEQ_OFF]) + X.MAX_LEN or not carry
    members = M.cut(text[carry:], 30000)
    first, last = np.maximum(idx[:, F.HDR_OFF] - 1 - carry, 0) // 30000, (idx[:, F.QUAL_OFF] + idx[:, F.QUAL_LEN] - carry) // 30000
    assert (last - first)[idx[:, F.HDR_OFF] > carry].max() >= 4                          # a record lies in five members or more
    got = eng.filter_bgzf_fastq(*M.batch_of(members), carry=text[:carry])
    ref = eng.filter_fastq(text)
    assert np.array_equal(got.idx, idx) and np.array_equal(ref.idx, idx) and got.consumed == ref.consumed == len(text)
    assert got.bad is None and got.text.tobytes() == text
    st = got.member_stats
    assert st["members"] == st["taken"] == len(members) and st["handed_back"] == 0
    same_results(got, fastq_want)
    same_results(ref, fastq_want)


# ---- the formatter -------------------------------------------------------------------------------------------------------------------

def fmt_want(text, idx, sel, kind, **kw):
    return bytes(F.format_records(text, idx, np.arange(len(idx)) if sel is None else sel, kind, **kw))


@pytest.mark.parametrize("kind", KINDS, ids=["fasta", "qual", "fastq"])
def test_format_uploaded_and_resident_are_fastio_formats_bytes(eng, kind):
    text, idx = X.fastq_text()
    n = len(idx)
    res = eng.filter_fastq(text)
    assert res.resident == eng.resident_text() > 0
    sels = (None, np.concatenate([np.arange(n)[::-1], [1, 1, 3, 0, 1]]))             # reversed, and with repeats of the longest
    for sel in sels:
        for max_len in (0, 40000, 65535):
            if sel is not None and max_len == 65535:
                continue
            w = fmt_want(text, idx, sel, kind, max_len=max_len)
            assert eng.format_text(text, idx, sel, kind=kind, max_len=max_len) == w, (max_len, "uploaded")
            assert eng.format_text(idx=res.idx, sel=sel, kind=kind, resident=res.resident, max_len=max_len) == w, (max_len, "resident")
    w = fmt_want(text, idx, None, kind)
    check_compressed(eng, eng.format_text(text, idx, kind=kind, bgzf=True), w)
    check_compressed(eng, eng.format_text(idx=res.idx, kind=kind, resident=res.resident, bgzf=True), w)
    assert eng.resident_text() == res.resident


@pytest.mark.parametrize("offsets", [(33, 33), (33, 64), (64, 33)], ids=["33_33", "33_64", "64_33"])
@pytest.mark.parametrize("nl", [b"\n", b"\r\n"], ids=["lf", "crlf"])
def test_format_every_quality_byte_at_every_lane_with_every_offset_pair(eng, offsets, nl):
    text, idx = X.fastq_text(nl, "every")
    assert X.every_byte_is_everywhere(text, idx)
    for clamp in (True, False):
        for kind in (F.FMT_QUAL, F.FMT_FASTQ):
            kw = dict(fastq_offset=offsets[0], out_offset=offsets[1], clamp_q0=clamp)
            assert eng.format_text(text, idx, kind=kind, **kw) == fmt_want(text, idx, None, kind, **kw), (clamp, kind)


def test_format_windows_of_50000_bytes_cross_the_longest_qual_record_four_times(eng, monkeypatch):
    text, idx = X.fastq_text(b"\n", "every")
    kw = dict(fastq_offset=0, out_offset=33)                 # values 33..126: two and three digits, the longest QUAL record there is
    w = fmt_want(text, idx, None, F.FMT_QUAL, **kw)
    lo, hi = (len(fmt_want(text, idx, np.arange(k), F.FMT_QUAL, **kw)) for k in (1, 2))
    assert (hi - 1) // 50000 - lo // 50000 >= 4              # window edges inside record 1
    monkeypatch.setenv("MPB_FORMAT_PIECE_BYTES", "50000")
    assert eng.format_text(text, idx, kind=F.FMT_QUAL, **kw) == w
    text, idx = X.fastq_text()
    for kind in KINDS:
        assert eng.format_text(text, idx, kind=kind) == fmt_want(text, idx, None, kind)


# ---- collapse ------------------------------------------------------------------------------------------------------------------------

def test_collapse_of_65535_base_sequences_uploaded_and_resident(eng):
    for c in X.collapse_cases():
        h, rep = collapse_inputs.want(c)
        got = eng.collapse_text(c["text"], c["idx"], max_len=c["max_len"])
        assert np.array_equal(got[0], h) and np.array_equal(got[1], rep), c["name"]
    text, idx = X.collapse_fastq()
    res = eng.filter_fastq(text)
    assert np.array_equal(res.idx, idx)
    for max_len in (0, 40000):
        h, rep = collapse_inputs.want(collapse_inputs.case("fastq", text, idx, max_len=max_len))
        assert len(set(rep.tolist())) == (8 if not max_len else 3)
        for got in (eng.collapse_text(text, idx, max_len=max_len), eng.collapse_text(resident=res.resident, n=len(idx), max_len=max_len)):
            assert np.array_equal(got[0], h) and np.array_equal(got[1], rep), max_len
    assert eng.resident_text() == res.resident


# ---- fasta + qual -----------------------------------------------------------------------------------------------------------------------

FA_WANT = {}


def fa_want(c):
    if c["name"] not in FA_WANT:
        FA_WANT[c["name"]] = FA.want(c)
    return FA_WANT[c["name"]]


def fa_cases():
    out = [X.fasta_qual_case("blank_lf"), X.fasta_qual_case("tab_lf", b"\t"), X.fasta_qual_case("blank_crlf", b" ", b"\r\n"),
           X.fasta_qual_case("tab_crlf", b"\t", b"\r\n"), X.fasta_qual_case("open_last_line", last_eol=False),
           X.fasta_qual_case("open_last_line_crlf", b" ", b"\r\n", last_eol=False), X.fasta_qual_case("not_final_open_last_line", last_eol=False, final=False)]
    # out_cap: room for the slots up to the longest record's last byte (by the host's index), and for one byte less
    row = fa_want(out[0])[1][X.THREE_AT]
    end = int(row[F.QUAL_OFF] + row[F.QUAL_LEN])
    out.append(X.fasta_qual_case("out_cap_before_longest", out_cap=end - 1))
    out.append(X.fasta_qual_case("out_cap_behind_longest", out_cap=end))
    return out


FA_CASES = fa_cases()


@pytest.mark.parametrize("c", FA_CASES, ids=[c["name"] for c in FA_CASES])
def test_the_fasta_qual_index_of_long_records_is_the_hosts(eng, c):
    wout, widx, wfc, wqc = fa_want(c)
    rc, out, idx, n, fc, qc, used, why, which, bad = raw_index(eng, c)
    assert rc == L.OK and why == 0 and (n, fc, qc, used) == (len(widx), wfc, wqc, len(wout))
    assert np.array_equal(out[:used], wout) and (out[used:] == 0xA5).all()
    assert np.array_equal(idx[:n], widx) and (idx[n:] == -7).all()
    want_n = {"out_cap_before_longest": X.THREE_AT, "out_cap_behind_longest": X.THREE_AT + 1, "not_final_open_last_line": X.ONE_AT}.get(c["name"], X.ONE_AT + 1)
    assert n == want_n


@pytest.mark.parametrize("c", X.fasta_qual_refusals(), ids=[c["name"] for c in X.fasta_qual_refusals()])
def test_a_refusal_beyond_byte_200000_of_a_line_keeps_its_record(eng, c):
    rc, out, idx, n, fc, qc, used, why, which, bad = raw_index(eng, c)
    assert rc == L.OK and (why, which, bad) == c["expect"]
    with pytest.raises(E.NotTaken) as e:
        eng.filter_fasta_qual(c["ftext"], c["qtext"])
    assert (e.value.why, e.value.which, e.value.bad_record) == c["expect"]


def test_filter_fasta_qual_equals_the_oracle_and_leaves_the_slots_resident(eng, oracle):
    c = X.fasta_qual_case("blank_lf")
    wout, widx, wfc, wqc = fa_want(c)
    n = len(widx)
    # The record of one-digit values alone (65535 bases of Q0..Q9, about 24,000 expected errors) needs more DP rows than the
    # 16384 there are -- the oracle takes 27,654, and most of a minute of one core for them: it has no result (NaN, rejected), as
    # tests/test_gpu_long_reads.py states the rule, and the oracle runs on the other records.
    assert n == X.ONE_AT + 1
    q, lens, flags = F.pack(wout, widx, None, 0, 0, stride=STRIDE)
    ee, ns, ps, rows = oracle.filter_batch(q[:X.ONE_AT], lens=lens[:X.ONE_AT], threads=16)
    assert 8192 < rows.max() < 16384 and not np.isnan(ee).any()
    res = eng.filter_fasta_qual(c["ftext"], c["qtext"])
    assert np.array_equal(res.text, wout) and np.array_equal(res.idx, widx) and (res.f_consumed, res.q_consumed) == (wfc, wqc)
    assert np.array_equal(bits(res.ee)[:X.ONE_AT], bits(ee)) and np.isnan(res.ee[X.ONE_AT]) and not res.passed[X.ONE_AT]
    assert np.array_equal(res.ns[:X.ONE_AT], ns) and res.ns[X.ONE_AT] == 0 and np.array_equal(res.passed[:X.ONE_AT], ps.astype(bool))
    assert np.array_equal(res.lens, lens) and np.array_equal(res.has_n, flags.astype(bool))
    gen = res.resident
    assert gen == eng.resident_text() > 0
    sel = np.concatenate([np.arange(n)[::-1], [X.THREE_AT, 1]])
    for kind in KINDS:
        for s, max_len in ((None, 0), (sel, 40000)):
            kw = dict(fastq_offset=0, out_offset=33, max_len=max_len)
            assert eng.format_text(idx=res.idx, sel=s, kind=kind, resident=gen, **kw) == fmt_want(wout, widx, s, kind, **kw), (kind, max_len)
    for max_len in (0, 40000):
        h, rep = collapse_inputs.want(collapse_inputs.case("slots", wout.tobytes(), widx, max_len=max_len))
        got = eng.collapse_text(resident=gen, n=n, max_len=max_len)
        assert np.array_equal(got[0], h) and np.array_equal(got[1], rep)
    assert eng.resident_text() == gen


# ---- the limit --------------------------------------------------------------------------------------------------------------------------

def test_a_record_of_65536_bases_is_indexed_and_refused_by_the_filters(eng, fastq_want):
    good, gidx = X.fastq_text()
    text, idx = X.too_long_text()
    same_as_host(eng, "65536 bases", text, 1, BIG)
    assert eng.fastq_index(text)[0][2, F.SEQ_LEN] == X.MAX_LEN + 1
    f, q = X.fasta_qual_too_long()
    wout, widx, wfc, wqc = FA.want(FA.case("too_long", f, q))
    out, fidx, fc, qc = eng.fasta_qual_index(f, q)
    assert np.array_equal(out, wout) and np.array_equal(fidx, widx) and (fc, qc) == (wfc, wqc) and fidx[1, F.SEQ_LEN] == X.MAX_LEN + 1
    for call in (lambda: eng.filter_fastq(text), lambda: eng.filter_fasta_qual(f, q)):
        res = eng.filter_fastq(good)
        assert res.resident == eng.resident_text() > 0
        with pytest.raises(ValueError, match="65535"):
            call()
        assert eng.resident_text() == 0                      # the earlier generation is no longer resident
        with pytest.raises(E.NotResident):
            eng.format_text(idx=res.idx, resident=res.resident)
        with pytest.raises(E.NotResident):
            eng.collapse_text(resident=res.resident, n=len(res.idx))
    with pytest.raises(ValueError, match="65535") as e:
        eng.filter_text(text, idx)
    assert e.value.bad_record == 2
    again = eng.filter_fastq(good)                           # the next good call on the same engine is right
    assert np.array_equal(again.idx, gidx)
    same_results(again, fastq_want)
    same_results(eng.filter_text(good, gidx), fastq_want)
