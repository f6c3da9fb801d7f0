"""BGZF FASTQ filtered where it inflates, on the GPU (include/moira_pb.h: mpb_filter_bgzf_fastq_host; Engine.filter_bgzf_fastq; the
CLI with --device_inflate, --device_index and --device_pack together).  The reference for every case is fastio.index(text) +
Engine.filter_text(text, idx) on text = carry + the zlib-inflated members: idx, consumed, bad, ee (as uint64), ns, passed, lens,
has_n and .text are compared with array_equal.  Members come from tests/helpers/inflate_inputs.py, texts from
tests/helpers/fastq_index_texts.py and the golden reads."""
import gzip
import os

import numpy as np
import pytest

from helpers import bgzf_fastq_inputs as M
from helpers import fastq_index_texts as X
from helpers import inflate_inputs as I
from moira_amd import cli
from moira_amd import engine as E
from moira_amd import fastio as F
from test_gpu_fastq_index import host_index

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def reads():
    """200 golden reads: text that members of one byte still cut into few enough members for a test."""
    return M.golden_text(200)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same(eng, members, carry=b"", final=True, max_records=None, text=True, batch=None, **kw):
    """One fused call against fastio.index + filter_text on carry + the zlib-inflated members."""
    batch = M.batch_of(members) if batch is None else batch
    whole = carry + M.inflated(batch)
    idx, consumed, bad = host_index(whole, final, X.BIG if max_records is None else max_records)
    want = eng.filter_text(whole, idx, **kw)
    got = eng.filter_bgzf_fastq(*batch, carry=carry, final=final, max_records=max_records, text=text, **kw)
    assert np.array_equal(got.idx, idx) and got.consumed == consumed
    assert (got.bad is None) == (bad is None)
    if bad is not None:
        assert (got.bad.kind, got.bad.header, got.bad.row.tolist()) == (bad[0], bad[1] if text else None, bad[2])
    assert np.array_equal(bits(got.ee), bits(want.ee)) and np.array_equal(got.ns, want.ns) and np.array_equal(got.passed, want.passed)
    assert np.array_equal(got.lens, want.lens) and np.array_equal(got.has_n, want.has_n)
    assert (got.n_pass, got.n_fail, got.n_overflow) == (want.n_pass, want.n_fail, want.n_overflow)
    if text:
        assert got.text.dtype == np.uint8 and got.text.tobytes() == whole
    else:
        assert got.text is None
    st = got.member_stats
    assert st["members"] == st["taken"] == len(batch[1]) and st["handed_back"] == 0
    return got


# ---- inputs the device takes ------------------------------------------------------------------------------------------------------

def test_golden_reads_by_both_compressors(eng, reads):
    got = same(eng, None, batch=M.scan(cli.bgzf_compress(reads)))
    assert len(got.ee) == 200 and 0 < got.n_pass < 200 and got.member_stats["dynamic_blocks"] >= 1
    same(eng, None, batch=M.scan(bytes(eng.bgzf_compress(reads))))
    same(eng, None, batch=M.scan(cli.bgzf_compress(reads)), poisson=True)
    same(eng, None, batch=M.scan(cli.bgzf_compress(reads)), max_len=100, lower_n_is_base=True)


@pytest.mark.parametrize("size", [1, 2, 3, 1000])
def test_members_that_end_mid_line_mid_record_and_on_record_ends(eng, reads, size):
    text = reads if size >= 3 else reads[:20000]
    members = M.cut(text, size)
    assert len(members) == (len(text) + size - 1) // size
    same(eng, members)


def test_stored_fixed_and_dynamic_members_in_one_call(eng, reads):
    a, b = len(reads) // 3, 2 * len(reads) // 3
    members = [I.frame(I.deflate(reads[:a], 0), reads[:a]), I.frame(I.deflate(reads[a:b], 6, 8, 4), reads[a:b]),      # 4: Z_FIXED
               M.member(reads[b:])]
    got = same(eng, members)
    st = got.member_stats
    assert st["stored_blocks"] >= 1 and st["fixed_blocks"] == 1 and st["dynamic_blocks"] == 1


def test_empty_members_one_member_and_no_member(eng, reads):
    half = len(reads) // 2
    empty = M.member(b"")
    same(eng, [M.member(reads[:half]), empty, M.member(reads[half:])])
    same(eng, [M.member(reads[:half]), M.member(reads[half:]), empty])
    same(eng, [M.member(reads[:60000])])
    same(eng, [empty])
    same(eng, [], carry=reads[:3000])
    same(eng, [], carry=reads[:3000], final=False)
    same(eng, [])


@pytest.mark.parametrize("n", range(18))
def test_a_carry_moves_every_member_through_all_alignments(eng, reads, n):
    """carry = the first n bytes of a record that the members continue: every out_off moves by n."""
    members = M.cut(reads[n:], 777)
    same(eng, members, carry=reads[:n])


def test_a_carry_of_whole_records(eng, reads):
    idx, consumed, _ = F.index(reads, True, 1000)
    at = int(idx[7, F.HDR_OFF]) - 1                          # the '@' of record 7
    assert reads[at:at + 1] == b"@"
    same(eng, M.cut(reads[at:], 5000), carry=reads[:at])


def test_final_or_not_and_an_unterminated_last_line(eng, reads):
    open_end = reads[:-1]
    for final in (False, True):
        same(eng, M.cut(open_end, 4096), final=final)
        same(eng, M.cut(reads, 4096), final=final)
        same(eng, M.cut(reads[:len(reads) // 2], 4096), final=final)


def test_max_records_cuts_the_call(eng, reads):
    got = same(eng, M.cut(reads, 4096), max_records=77)
    assert len(got.ee) == 77 and got.consumed < len(reads)
    same(eng, M.cut(reads, 4096), max_records=0)


def test_more_records_than_the_guess_asks_once_more(eng):
    many = b"@\nA\n+\nI\n" * 3000
    got = same(eng, M.cut(many, 4000))
    assert len(got.ee) == 3000


def test_each_bad_record_kind_with_the_records_before_it_filtered(eng):
    good = X.records(30, 61, lo=20, hi=120)
    seen = set()
    for kind, bad in X.BAD.items():
        text = b"".join(good[:20]) + bad + b"".join(good[20:])
        got = same(eng, M.cut(text, 500))
        assert len(got.ee) == 20 and got.bad is not None and got.bad.header == "bad"
        seen.add(got.bad.kind)
        lean = same(eng, M.cut(text, 500), text=False)
        assert lean.bad.kind == got.bad.kind and lean.bad.header is None and lean.bad.row.tolist() == got.bad.row.tolist()
    assert seen == {F.REC_EMPTY_SEQ, F.REC_EMPTY_QUAL, F.REC_LENGTH_MISMATCH}


def test_without_the_text(eng, reads):
    got = same(eng, M.cut(reads, 30000), text=False)
    assert got.text is None and len(got.ee) == 200


def test_into_the_callers_own_text_buffer(eng, reads):
    batch = M.batch_of(M.cut(reads, 30000))
    want = eng.filter_bgzf_fastq(*batch)
    buf = np.full(len(reads) + 100, 0x5a, np.uint8)
    got = eng.filter_bgzf_fastq(*batch, text=buf)
    assert np.shares_memory(got.text, buf) and got.text.tobytes() == reads == buf[:len(reads)].tobytes() and (buf[len(reads):] == 0x5a).all()
    assert np.array_equal(bits(got.ee), bits(want.ee)) and np.array_equal(got.idx, want.idx)
    with pytest.raises(ValueError, match="text must be a contiguous uint8 array of at least"):
        eng.filter_bgzf_fastq(*batch, text=buf[:100])


def test_a_quality_out_of_range_is_the_same_valueerror(eng):
    good = X.records(30, 44)
    text = b"".join(good[:17]) + X.rec(b"x", b"ACG", b"I I") + b"".join(good[17:])
    idx, _, _ = F.index(text, True, 100)
    with pytest.raises(ValueError) as want:
        eng.filter_text(text, idx)
    with pytest.raises(ValueError) as got:
        eng.filter_bgzf_fastq(*M.batch_of(M.cut(text, 300)))
    assert str(got.value) == str(want.value) and got.value.bad_record == want.value.bad_record == 17


# ---- refusals ---------------------------------------------------------------------------------------------------------------------

def handed_back(eng, members, first, why):
    sentinel = 0x5a
    with pytest.raises(E.MembersNotTaken) as e:
        eng.filter_bgzf_fastq(*M.batch_of(members))
    assert e.value.first == first and int(e.value.why[first]) == why
    assert e.value.done.tolist() == [0 if k == first else 1 for k in range(len(members))]
    # no result array is touched: the C entry, with arrays of our own
    import ctypes as C
    data, offs, sizes, out_offs = M.batch_of(members)
    cap = 64
    arrs = [np.full(cap * 6, sentinel, np.int64), np.full(cap, sentinel, np.float64), np.full(cap, sentinel, np.int32),
            np.full(cap, sentinel, np.uint8), np.full(cap, sentinel, np.int32), np.full(cap, sentinel, np.uint8),
            np.full(int(out_offs[-1]) + 1, sentinel, np.uint8)]
    idx, ee, ns, ps, lens, flags, text = arrs
    done, mwhy = np.zeros(len(members), np.uint8), np.zeros(len(members), np.uint8)
    fb, n, consumed, bad, fw = C.c_int64(-5), C.c_int64(-5), C.c_int64(-5), C.c_int32(-5), C.c_int32(-5)
    params = eng.params()
    rc = eng.lib.mpb_filter_bgzf_fastq_host(eng.ctx, None, 0, data.ctypes.data, len(data), offs.ctypes.data, sizes.ctypes.data,
                                            out_offs.ctypes.data, len(members), 1, 1 << 40, 0, text.ctypes.data, len(text),
                                            done.ctypes.data, mwhy.ctypes.data, C.byref(fb), None, idx.ctypes.data, cap, C.byref(n),
                                            C.byref(consumed), C.byref(bad), C.byref(fw), 33, 0, C.byref(params), 0, ee.ctypes.data,
                                            ns.ctypes.data, ps.ctypes.data, lens.ctypes.data, flags.ctypes.data, None, None)
    assert rc == 0 and fb.value == first and n.value == 0 and int(mwhy[first]) == why
    assert all((a == np.full(1, sentinel, a.dtype)[0]).all() for a in arrs)


def test_a_wrong_crc_among_good_members_hands_the_batch_back(eng):
    good, _ = I.neighbour()
    wrong = [m for name, m, why in I.crafted_invalid() if name == "wrong_crc"][0]
    handed_back(eng, [good, good, wrong, good], 2, I.CRC)
    handed_back(eng, [wrong, good], 0, I.CRC)


def test_a_flipped_payload_bit_in_a_stored_member_is_seen_by_the_device_crc_alone(eng):
    """The stored member's stream is still a valid stream of the stated length: only the CRC-32 of its text can tell."""
    good, text = I.neighbour()
    stored = bytearray(I.frame(I.deflate(text, 0), text))
    at = I.parse(bytes(stored))[0] + 5 + 100                 # byte 100 of the payload, behind the block's five header bytes
    assert stored[at] == text[100]
    stored[at] ^= 0x10
    handed_back(eng, [good, bytes(stored), good], 1, I.CRC)


def test_a_member_the_device_does_not_take_keeps_its_reason(eng):
    good, _ = I.neighbour()
    by = {name: (m, why) for name, m, why in I.crafted_invalid()}
    for name in ("btype3", "cut_mid_symbol", "no_bc_subfield"):
        m, why = by[name]
        assert why in (I.BLOCK_TYPE, I.TRUNCATED, I.HEADER)
        handed_back(eng, [good, m, good], 1, why)


def test_a_non_ascii_byte_is_the_index_refusal(eng, reads):
    text = reads[:5000] + b"\xe9" + reads[5000:]
    with pytest.raises(E.NotTaken) as e:
        eng.filter_bgzf_fastq(*M.batch_of(M.cut(text, 3000)))
    assert e.value.why == 1


def test_the_kernels_show_in_the_timing_table(eng, reads):
    eng.timing(True)
    eng.timing_reset()
    eng.filter_bgzf_fastq(*M.batch_of(M.cut(reads, 30000)))
    t = eng.kernel_times()
    eng.timing(False)
    assert t["bgzf_inflate"][1] == 1 and t["fq_lines"][1] == 1 and t["fq_rows"][1] == 1 and t["pack_text"][1] >= 1, t


# ---- the CLI: --device_inflate, --device_index and --device_pack together ---------------------------------------------------------

def run_cli(tmp_path, name, src, on):
    """-> (the files, the exception or None, the log, the fused calls the engine saw as (members, records))."""
    import io
    from test_cli_golden import reference_args
    a = reference_args(paired=False, forward_fastq=src, output_prefix=str(tmp_path / name), device_pack=on, device_index=on,
                       collapse=False, processors=4)
    a.device_inflate = on
    be = cli.make_gpu_backend(None)
    seen = []
    inner = be.engine.filter_bgzf_fastq

    def fused(data, offs, *x, **kw):
        try:
            r = inner(data, offs, *x, **kw)
        except Exception as e:                               # noqa: B902 -- recorded, and the consumer's to take
            seen.append((len(offs), type(e).__name__))
            raise
        seen.append((len(offs), len(r.idx)))
        return r
    be.engine.filter_bgzf_fastq = fused
    log, err = io.StringIO(), None
    try:
        try:
            assert cli.main(a, backend=be, out=log) == 0
        except OSError as e:
            err = e
    finally:
        be.engine.close()
    files = {p.split(".", 1)[1]: open(os.path.join(str(tmp_path), p), "rb").read()
             for p in sorted(os.listdir(str(tmp_path))) if p.startswith(name + ".")}
    return files, err, log.getvalue(), seen


def test_cli_bgzf_input_is_identical_with_the_three_switches(tmp_path):
    text = M.golden_text()
    src = str(tmp_path / "in.fastq.gz")
    with open(src, "wb") as f:
        f.write(cli.bgzf_compress(text, 4) + cli.BGZF_EOF)
    off, err_off, _, seen_off = run_cli(tmp_path, "off", src, False)
    on, err_on, log, seen_on = run_cli(tmp_path, "on", src, True)
    assert err_off is None and err_on is None and seen_off == []
    assert sum(n for _, n in seen_on) == 1000 and sum(m for m, _ in seen_on) == len(text) // cli.BGZF_DATA + 2      # every member, the end marker too
    assert off.keys() == on.keys() and len(off) >= 2 and off == on and "--device_" not in log


def test_cli_plain_gzip_input_is_identical_with_the_three_switches(tmp_path):
    src = os.path.join(M.GOLD, "test1.fastq.gz")
    assert open(src, "rb").read()[12:14] != b"BC"            # one plain gzip member: no batch of members comes of it
    off, _, _, _ = run_cli(tmp_path, "off", src, False)
    on, err, log, seen = run_cli(tmp_path, "on", src, True)
    assert err is None and seen == [] and off == on and len(on) >= 2


def test_cli_a_corrupted_member_ends_with_the_host_decoders_error(tmp_path):
    text = M.golden_text()
    members = M.cut(text, 40000)
    bad = bytearray(members[3])
    bad[len(bad) // 2] ^= 0x04                               # somewhere inside the deflate stream
    src = str(tmp_path / "bad.fastq.gz")
    with open(src, "wb") as f:
        f.write(b"".join(members[:3]) + bytes(bad) + b"".join(members[4:]))
    off, err_off, _, _ = run_cli(tmp_path, "off", src, False)
    on, err_on, log, seen = run_cli(tmp_path, "on", src, True)
    assert isinstance(err_off, OSError) and isinstance(err_on, OSError) and str(err_on) == str(err_off) and "BGZF block 3" in str(err_on)
    assert seen == [(len(members), "MembersNotTaken")]
    assert log.count("--device_inflate with --device_index: the device did not take a batch of members") == 1
