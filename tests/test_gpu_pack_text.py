"""k_pack_text and the entries around it on the GPU (include/moira_pb.h: mpb_pack_text_device, mpb_filter_text_host; the CLI's
--device_pack).  mio_pack (through fastio.pack) is the reference everywhere: the WHOLE matrix including its padding, the lengths
and the flags are compared with array_equal; filter results are compared bit for bit (ee as uint64, NaN included) with the
host-packed run.  The host-only half (mpb_text_rows, the chunk code against mio_pack on the CPU): tests/test_text_rows.py."""
import bz2
import ctypes as C
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

from moira_amd import cli
from moira_amd import engine as E
from moira_amd import fastio as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
I64_MAX = np.iinfo(np.int64).max
SWEEP_LENGTHS = (1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 300)


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(0)
    yield e
    e.close()


# ---- building texts and their indices by hand -------------------------------------------------------------------------------

class Text:
    """A text laid out line by line at chosen byte residues, with its record index (HDR columns unused: 0)."""

    def __init__(self, lead=0):
        self.buf = bytearray(b"#" * lead)
        self.rows = []

    def pad_to(self, residue, filler=b"N"):
        while len(self.buf) % 16 != residue:
            self.buf += filler

    def add(self, seq, qual, seq_res=None, qual_res=None):
        assert len(seq) == len(qual)
        if seq_res is not None:
            self.pad_to(seq_res, b"n")
        so = len(self.buf)
        self.buf += seq
        self.buf += b"\n"
        if qual_res is not None:
            self.pad_to(qual_res, b"\xff")
        qo = len(self.buf)
        self.buf += qual
        self.rows.append((0, 0, so, len(seq), qo, len(qual)))
        return len(self.rows) - 1

    def done(self):
        return bytes(self.buf), np.array(self.rows, np.int64).reshape(-1, 6)


def random_record(rng, ln, offset=33, p_amb=0.03):
    seq = rng.choice(np.frombuffer(b"ACGTNn", np.uint8), ln, p=[(1 - 2 * p_amb) / 4] * 4 + [p_amb] * 2).astype(np.uint8).tobytes()
    qv = rng.integers(0, 42, ln)
    qv[rng.random(ln) < 0.05] = 0                                               # Q0 -> 1
    return seq, (qv + offset).astype(np.uint8).tobytes()


def run_pack(eng, text, idx, sel=None, stride=None, offset=33, lower=False, max_len=0, fill=0xFF):
    """k_pack_text through Engine.pack_text_device -> (q uint8[n, stride], lens, flags bool, status int64[2]).  The text buffer has
    exactly round_up(len(text), 16) bytes (at least 16); what lies past the text is `fill`; every output byte starts as 0xAB."""
    if stride is None:
        stride = (max(E.text_rows(idx, sel, text_bytes=len(text), max_len=max_len)[1], 1) + 127) // 128 * 128
    rows, _ = E.text_rows(idx, sel, text_bytes=len(text), max_len=max_len, stride=stride)
    n = len(rows)
    cap = max((len(text) + 15) // 16 * 16, 16)
    host = np.full(cap, fill, np.uint8)
    host[:len(text)] = np.frombuffer(text, np.uint8)
    bufs = []

    def dev(arr):
        arr = np.ascontiguousarray(arr)
        b = eng.alloc(max(arr.nbytes, 16)).upload(arr)
        bufs.append(b)
        return b
    d_text, d_rows = dev(host), dev(rows if n else np.zeros(1, E.TEXT_ROW_DTYPE))
    d_q, d_len, d_flags = dev(np.full(max(n, 1) * stride, 0xAB, np.uint8)), dev(np.full(max(n, 1), -9, np.int32)), dev(np.full(max(n, 1), 0xAB, np.uint8))
    d_status = dev(np.full(2, I64_MAX, np.int64))
    try:
        eng.pack_text_device(d_text, len(text), d_rows, n, stride, d_q, d_len, d_flags, d_status, fastq_offset=offset, lower_n_is_base=lower)
        eng.synchronize()
        q = d_q.download(np.uint8, n * stride).reshape(n, stride)
        lens, flags, status = d_len.download(np.int32, n), d_flags.download(np.uint8, n), d_status.download(np.int64, 2)
    finally:
        for b in bufs:
            b.free()
    assert set(np.unique(flags)) <= {0, 1}
    return q, lens, flags.astype(bool), status


def mio_pack_raw(text, idx, sel, offset, max_len, lower, stride):
    """mio_pack itself -> (rc, bad_record, message, q, lens, flags)."""
    lib = F.load()
    idx = np.ascontiguousarray(idx)
    sel = np.ascontiguousarray(np.arange(len(idx)) if sel is None else sel, np.int64)
    n = len(sel)
    q, lens, flags = np.zeros((n, stride), np.uint8), np.zeros(n, np.int32), np.zeros(n, np.uint8)
    bad = C.c_int64(-1)
    rc = lib.mio_pack(text, idx.ctypes.data, sel.ctypes.data, n, offset, max_len, 1 if lower else 0, stride, q.ctypes.data,
                      lens.ctypes.data, flags.ctypes.data, C.addressof(bad))
    return rc, bad.value, lib.mio_last_error().decode() if rc else "", q, lens, flags.astype(bool)


def check_against_mio_pack(eng, text, idx, sel=None, stride=None, offset=33, lower=False, max_len=0, fill=0xFF):
    q, lens, flags, status = run_pack(eng, text, idx, sel, stride, offset, lower, max_len, fill)
    rq, rlens, rflags = F.pack(text, idx, sel, offset, max_len, lower, stride=q.shape[1])
    assert status.tolist() == [I64_MAX, I64_MAX]
    assert np.array_equal(q, rq) and np.array_equal(lens, rlens) and np.array_equal(flags, rflags)
    return q, lens, flags


# ---- 1. alignment sweep -------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def sweep():
    """256 records: the sequence line at every residue 0..15 and the quality line at every residue 0..15, independently."""
    rng = np.random.default_rng(1)
    t = Text(lead=3)
    k = 0
    for sr in range(16):
        for qr in range(16):
            seq, qual = random_record(rng, SWEEP_LENGTHS[k % len(SWEEP_LENGTHS)])
            t.add(seq, qual, sr, qr)
            k += 1
    text, idx = t.done()
    assert {(int(r[2]) % 16, int(r[4]) % 16) for r in idx} == {(a, b) for a in range(16) for b in range(16)}
    assert set(idx[:, 5].tolist()) == set(SWEEP_LENGTHS)
    return text, idx


@pytest.mark.parametrize("stride,max_len", [(128, 128), (384, 0), (304, 0)])
def test_alignment_sweep(eng, sweep, stride, max_len):
    """(Stride 128 cannot hold the reads of 129 and 300 bases: they are packed truncated to 128, mio_pack's max_len rule.)"""
    text, idx = sweep
    q, lens, flags = check_against_mio_pack(eng, text, idx, stride=stride, max_len=max_len)
    assert flags.any() and not flags.all() and (q == 255).any() and (q == 0).any()


# ---- 2. the byte rules in every byte lane -----------------------------------------------------------------------------------

@pytest.mark.parametrize("lower", [False, True], ids=["n_is_ambiguous", "n_is_base"])
@pytest.mark.parametrize("offset", [33, 64])
def test_byte_rules_in_every_byte_lane(eng, offset, lower):
    t = Text(lead=5)
    ln = 40
    for i in range(16):
        for what in ("N", "n", "q0"):
            seq, qual = bytearray(b"ACGT" * 10), bytearray([offset + 30] * ln)
            for pos in (i, i + 16):                                             # the lane of byte i, in two chunks of the row
                if what == "q0":
                    qual[pos] = offset
                else:
                    seq[pos] = ord(what)
            t.add(bytes(seq), bytes(qual))
    t.add(b"N" * ln, bytes([offset + 2] * ln))                                  # a record that is all N
    t.add(b"n" * 17, bytes([offset] * 17))
    text, idx = t.done()
    q, lens, flags = check_against_mio_pack(eng, text, idx, offset=offset, lower=lower)
    for i in range(16):
        rN, rn, r0 = q[3 * i], q[3 * i + 1], q[3 * i + 2]
        assert rN[i] == 0 and rN[i + 16] == 0 and rn[i] == (30 if lower else 255) and r0[i] == 1 and r0[i + 16] == 1
        assert flags[3 * i] and not flags[3 * i + 1] and not flags[3 * i + 2]
    assert not q[-2].any() and flags[-2] and not flags[-1] and (q[-1, :17] == (1 if lower else 255)).all()


# ---- 3. truncation ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("max_len", [1, 16, 299, 300, 301])
def test_truncation(eng, max_len):
    rng = np.random.default_rng(3)
    t = Text(lead=1)
    for ln in (300, 7, 16, 17, 250, 300, 1):
        t.add(*random_record(rng, ln, p_amb=0.1))
    text, idx = t.done()
    q, lens, flags = check_against_mio_pack(eng, text, idx, max_len=max_len)
    assert lens.tolist() == [min(ln, max_len) for ln in (300, 7, 16, 17, 250, 300, 1)]
    assert q.shape[1] % 128 == 0 and not q[:, min(max_len, q.shape[1]):].any()                 # the tail of every row is zero
    for k in range(len(lens)):
        assert not q[k, lens[k]:].any()


# ---- 4. batch edges -------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def batch257():
    rng = np.random.default_rng(4)
    t = Text(lead=2)
    for k in range(257):
        t.add(*random_record(rng, int(rng.integers(0, 140))))
    return t.done()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_batch_edges(eng, batch257, n):
    text, idx = batch257
    idx = idx[:n]
    rng = np.random.default_rng(n)
    check_against_mio_pack(eng, text, idx)
    check_against_mio_pack(eng, text, idx, sel=np.arange(n)[::-1])
    check_against_mio_pack(eng, text, idx, sel=np.arange(0, n, 3))
    check_against_mio_pack(eng, text, idx, sel=rng.integers(0, n, n + 9))
    q, lens, flags, status = run_pack(eng, text, idx, sel=[], stride=128)      # nothing to do is not an error
    assert q.shape == (0, 128) and status.tolist() == [I64_MAX, I64_MAX]


# ---- 5. nothing past text_bytes reaches an output --------------------------------------------------------------------------

@pytest.mark.parametrize("residue", range(16))
def test_no_dependence_on_bytes_past_the_text(eng, residue):
    rng = np.random.default_rng(50 + residue)
    t = Text(lead=0)
    for ln in (33, 5, 64, 18):
        t.add(*random_record(rng, ln))
    t.pad_to((residue - 41) % 16, b"\xff")                                 # 20 bases, a newline, 20 qualities follow
    t.add(*random_record(rng, 20))                                              # the last quality line ends at the last byte
    text, idx = t.done()
    assert len(text) % 16 == residue and idx[-1, 4] + idx[-1, 5] == len(text)
    a = check_against_mio_pack(eng, text, idx, fill=0xFF)
    b = check_against_mio_pack(eng, text, idx, fill=ord("N"))
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


# ---- 6. bad qualities: a validated error path ---------------------------------------------------------------------------------

def bad_text(kind, k, n=9):
    """n records of 50 bases; record k carries a quality character below 33 ("below"), the byte 255 ("above": Q 255 at offset 0) or
    both.  (One call cannot report both kinds for one record: a byte c is below the offset or 254 above it, never both, and no
    offset makes one byte of the text the first and another the second -- above needs offset 0, where nothing is below.  The
    record with both is therefore checked at offset 33, where it is a "positive values" record, and at offset 0, where it is a
    "maximum 254" one.)"""
    rng = np.random.default_rng(6)
    t = Text(lead=7)
    for i in range(n):
        seq, qual = random_record(rng, 50)
        qual = bytearray(qual)
        if i == k:
            if kind in ("below", "both"):
                qual[37] = 20
            if kind in ("above", "both"):
                qual[11] = 255
        t.add(seq, bytes(qual))
    return t.done()


@pytest.mark.parametrize("kind,k,offset", [("below", 0, 33), ("below", 4, 33), ("below", 8, 33), ("above", 4, 0), ("both", 4, 33), ("both", 4, 0),
                                           ("below", 2, 64)])
def test_bad_qualities_are_reported_not_faulted(eng, kind, k, offset):
    text, idx = bad_text(kind, k)
    n = len(idx)
    rc, bad, msg, _, _, _ = mio_pack_raw(text, idx, None, offset, 0, False, 128)
    first_bad = k if offset != 64 else 0                                        # (at offset 64 every record of this text is below)
    assert rc == F.E_RANGE and bad == first_bad
    q, lens, flags, status = run_pack(eng, text, idx, stride=128, offset=offset)
    positive = "positive" in msg
    assert min(status) == bad and (status[0] == bad) == positive
    if offset != 64:
        assert status.tolist() == ([k, I64_MAX] if positive else [I64_MAX, k])
    # every record that is clean by itself is packed as the reference packs it
    clean = 0
    for j in range(n):
        rc1, _, _, rq, rl, rf = mio_pack_raw(text, idx, [j], offset, 0, False, 128)
        if rc1 == 0:
            clean += 1
            assert np.array_equal(q[j], rq[0]) and lens[j] == rl[0] and flags[j] == rf[0]
    assert clean == (n - 1 if offset != 64 else 0)
    assert lens.tolist() == [50] * n                                            # the bad record's row is written too (Q1 / Q254)
    # filter_text: the library's error is mio_pack's, and no result array is touched
    out = (np.full(n, -7.5), np.full(n, -7, np.int32), np.full(n, 7, np.uint8), np.full(n, -7, np.int32), np.full(n, 7, np.uint8))
    with pytest.raises(ValueError) as e:
        eng.filter_text(text, idx, fastq_offset=offset, out=out)
    assert str(e.value) == msg and e.value.bad_record == bad
    assert (out[0] == -7.5).all() and (out[1] == -7).all() and (out[2] == 7).all() and (out[3] == -7).all() and (out[4] == 7).all()
    with pytest.raises(ValueError) as e:                                        # ... also when the bad record is the only one selected
        eng.filter_text(text, idx, sel=[first_bad], fastq_offset=offset, poisson=True, lower_n_is_base=True)
    assert str(e.value) == msg and e.value.bad_record == 0


def test_filter_text_refuses_what_the_text_cannot_hold(eng):
    text, idx = bad_text("none", -1)
    bad = idx.copy()
    bad[3, 4] = len(text) - 49                                                  # the quality line ends one byte past the text
    with pytest.raises(ValueError) as e:
        eng.filter_text(text, bad)
    assert e.value.bad_record == 3
    with pytest.raises(ValueError):
        eng.filter_text(text, idx, fastq_offset=300)
    r = eng.filter_text(text, idx, sel=[])
    assert len(r.ee) == 0 and r.n_pass == 0


# ---- 7. end to end on the golden reads ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def golden_inputs():
    """{"reads": the 1,000 records of test1.fastq.gz, "contigs": what mct_contigs_from_fastq makes of the paired golden inputs},
    each as (buffer, index)."""
    from moira_amd import contig as CT
    fbuf = gzip.open(os.path.join(GOLD, "test1.fastq.gz"), "rb").read()
    rbuf = bz2.open(os.path.join(GOLD, "test2.fastq.bz2"), "rb").read()
    fidx, _, err = F.index(fbuf, True, 100000)
    ridx, _, err2 = F.index(rbuf, True, 100000)
    assert err is None and err2 is None and len(fidx) == 1000 and len(ridx) >= 400
    m = min(len(fidx), len(ridx))
    cbuf, cidx, aux = CT.contigs_from_fastq(fbuf, fidx[:m], rbuf, ridx[:m], 33, threads=4)
    return {"reads": (fbuf, fidx), "contigs": (cbuf, cidx)}


def same_results(r, ref, lens, has_n):
    assert np.array_equal(r.ee.view(np.uint64), ref.ee.view(np.uint64))        # bit for bit, NaN included
    assert np.array_equal(r.ns, ref.ns) and np.array_equal(r.passed, ref.passed)
    assert np.array_equal(r.lens, lens) and np.array_equal(r.has_n, has_n)
    assert r.n_pass == ref.n_pass == int(ref.passed.sum())


CASES = {"default": dict(), "truncate100": dict(max_len=100), "round": dict(round_=True), "ignore": dict(ambigs="ignore"),
         "disallow": dict(ambigs="disallow"), "treat_as_errors": dict(ambigs="treat_as_errors"), "odd_reversed": dict(sel="odd")}


@pytest.mark.parametrize("poisson", [False, True], ids=["poisson_binomial", "poisson"])
@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("which", ["reads", "contigs"])
def test_filter_text_equals_the_host_packed_run(eng, golden_inputs, which, case, poisson):
    buf, idx = golden_inputs[which]
    kw = dict(CASES[case])
    max_len = kw.pop("max_len", 0)
    sel = np.arange(1, len(idx), 2)[::-1].copy() if kw.pop("sel", None) else None
    lower = poisson                                  # the Poisson function scores a lower-case n as a base (the CLI packs it so)
    q, lens, has_n = F.pack(buf, idx, sel, 33, max_len, lower)
    ref = (eng.filter_poisson if poisson else eng.filter)(q, lens=lens, **kw)
    r = eng.filter_text(buf, idx, sel, max_len=max_len, lower_n_is_base=lower, poisson=poisson, **kw)
    same_results(r, ref, lens, has_n)
    assert len(lens) == (500 if sel is not None else 1000)


def test_filter_text_with_the_poisson_device_tail_is_the_resident_entry(eng, golden_inputs):
    """With MPB_FLAG_POISSON_DEVICE_TAIL the entry runs mpb_filter_poisson_device on each piece: the host entry's results with
    the same flag (decisions exact, ee within the device tail's contract)."""
    buf, idx = golden_inputs["reads"]
    q, lens, has_n = F.pack(buf, idx, None, 33, 0, True)
    ref = eng.filter_poisson(q, lens=lens, poisson_device_tail=True)
    r = eng.filter_text(buf, idx, lower_n_is_base=True, poisson=True, poisson_device_tail=True)
    assert np.array_equal(r.passed, ref.passed) and np.array_equal(r.ns, ref.ns)
    assert np.allclose(r.ee, ref.ee, rtol=1e-9, atol=0, equal_nan=True)


# ---- 8. through the ragged narrow pass; 9. pieces ------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def tiled(eng, golden_inputs):
    """The golden reads tiled to 5,000 records (more than one 4096-read sort window of the ragged pass) and the host-packed run."""
    buf, idx = golden_inputs["reads"]
    sel = np.arange(5000) % len(idx)
    q, lens, has_n = F.pack(buf, idx, sel, 33, 0, False)
    return buf, idx, sel, lens, has_n, eng.filter(q, lens=lens)


@pytest.mark.parametrize("rows", [2, 3, 4])
def test_filter_text_through_the_ragged_narrow_pass(eng, tiled, rows):
    buf, idx, sel, lens, has_n, ref = tiled
    eng.timing(True)
    eng.timing_reset()
    try:
        r = eng.filter_text(buf, idx, sel, narrow_rows=rows)
        times = eng.kernel_times()
    finally:
        eng.timing(False)
    same_results(r, ref, lens, has_n)
    assert eng.last_path()["narrow_rows"] == rows
    assert times["pack_text"][1] == 1                                          # one launch of k_pack_text per piece: one piece


def test_pieces(eng, tiled, monkeypatch):
    buf, idx, sel, lens, has_n, ref = tiled
    stride = (int(lens.max()) + 127) // 128 * 128
    monkeypatch.setenv("MPB_TEXT_PIECE_BYTES", str(1500 * stride))              # 5,000 rows in pieces of 1,500: four pieces
    eng.timing(True)
    eng.timing_reset()
    try:
        r = eng.filter_text(buf, idx, sel)
        rp = eng.filter_text(buf, idx, sel, poisson=True, lower_n_is_base=True)
        times = eng.kernel_times()
    finally:
        eng.timing(False)
    assert times["pack_text"][1] == 8                                           # four pieces per call
    same_results(r, ref, lens, has_n)
    monkeypatch.delenv("MPB_TEXT_PIECE_BYTES")
    one = eng.filter_text(buf, idx, sel, poisson=True, lower_n_is_base=True)
    assert np.array_equal(rp.ee.view(np.uint64), one.ee.view(np.uint64)) and np.array_equal(rp.passed, one.passed)
    assert np.array_equal(rp.ns, one.ns) and rp.n_pass == one.n_pass


@pytest.mark.parametrize("poisson", [False, True], ids=["poisson_binomial", "poisson"])
def test_bad_qualities_in_later_pieces_are_reported_in_sel_order(eng, monkeypatch, poisson):
    """A call that runs in several pieces reports the first bad record in sel order with mio_pack's message, wherever in its piece
    it lies: bad records in the second and third piece, the later one at a smaller position inside its piece, both kinds (each at
    the offset that makes it one), and records that come first in sel order only through sel."""
    rng = np.random.default_rng(12)
    t = Text(lead=9)
    n = 40
    for i in range(n):
        seq, qual = random_record(rng, 50, offset=0, p_amb=0)
        qual = bytearray(v + 40 for v in qual)                                  # clean at offset 0 and at offset 33
        t.add(seq, bytes(qual))
    text, idx = t.done()
    monkeypatch.setenv("MPB_TEXT_PIECE_BYTES", str(10 * 128))                   # stride 128: pieces of 10 rows, four pieces
    kw = dict(poisson=poisson, lower_n_is_base=poisson)
    assert eng.filter_text(text, idx, fastq_offset=33, **kw).lens.tolist() == [50] * n

    def planted(spots):
        b = bytearray(text)
        for rec, value in spots:
            b[idx[rec, 4] + 23] = value
        return bytes(b)
    # (offset, planted bytes, sel): at offset 33 a byte 20 is below; at offset 0 a byte 255 is above
    for offset, spots, sel in ((33, [(17, 20)], None), (33, [(17, 20), (22, 20)], None), (33, [(25, 20), (31, 20)], None),
                               (0, [(17, 255), (22, 255)], None), (0, [(39, 255)], None),
                               (33, [(3, 20)], np.arange(n)[::-1].copy()), (33, [(17, 20), (2, 20)], (np.arange(n) + 5) % n)):
        bad_text_ = planted(spots)
        rc, bad, msg, _, _, _ = mio_pack_raw(bad_text_, idx, sel, offset, 0, poisson, 128)
        assert rc == F.E_RANGE and bad >= 10                                    # the first bad record lies in a later piece
        out = (np.full(n, -7.5), np.full(n, -7, np.int32), np.full(n, 7, np.uint8), np.full(n, -7, np.int32), np.full(n, 7, np.uint8))
        with pytest.raises(ValueError) as e:
            eng.filter_text(bad_text_, idx, sel, fastq_offset=offset, out=out, **kw)
        assert (e.value.bad_record, str(e.value)) == (bad, msg), (offset, spots)
        assert (out[0] == -7.5).all() and (out[1] == -7).all() and (out[2] == 7).all() and (out[3] == -7).all() and (out[4] == 7).all()


def test_pack_text_status_counts_from_zero_in_the_resident_entry(eng):
    """mpb_pack_text_device reports positions in ITS rows (the base of the host entry's pieces is not part of the ABI)."""
    text, idx = bad_text("below", 8)
    q, lens, flags, status = run_pack(eng, text, idx, sel=[7, 8, 8], stride=128)
    assert status.tolist() == [1, I64_MAX]


# ---- 10. the CLI ---------------------------------------------------------------------------------------------------------------

KINDS = ("good.fasta", "good.qual", "good.names", "bad.fasta", "bad.qual", "bad.names")


def counting_backend():
    be = cli.make_gpu_backend(None)
    calls = []
    inner = be.text

    def text(*a, **kw):
        r = inner(*a, **kw)
        calls.append(len(a[1]))                                                 # (chunks the device took: counted once it has returned)
        return r
    be.text = text
    return be, calls


@pytest.mark.parametrize("paired", [False, True], ids=["forward", "paired"])
def test_cli_golden_commands_with_device_pack(tmp_path, paired):
    from test_cli_golden import reference_args, same_files
    got = []
    for on in (False, True):
        out = str(tmp_path / ("on" if on else "off"))
        a = reference_args(paired=paired, forward_fastq=os.path.join(GOLD, "test1.fastq.gz"), output_prefix=out,
                           reverse_fastq=os.path.join(GOLD, "test2.fastq.bz2") if paired else None)
        a.device_pack = on
        be, calls = counting_backend()
        try:
            assert cli.main(a, backend=be, out=open(os.devnull, "w")) == 0
        finally:
            be.engine.close()
        assert (len(calls) >= 1) == on and (not on or sum(calls) == 1000)       # one call per chunk, every record (or contig)
        same_files(out, "paired" if paired else "forward")
        files = sorted(p for p in os.listdir(tmp_path) if p.startswith(os.path.basename(out) + "."))
        got.append({p.split(".", 1)[1]: open(os.path.join(str(tmp_path), p), "rb").read() for p in files})
    assert got[0].keys() == got[1].keys() and all("qc." + k in got[0] for k in KINDS) and got[0] == got[1]


def test_cli_bad_quality_character_ends_the_same_way(tmp_path):
    """One quality character below the offset: the same exception text and exit status with and without the switch."""
    fq = tmp_path / "bad.fastq"
    rng = np.random.default_rng(10)
    with open(fq, "wb") as f:
        for k in range(30):
            seq, qual = random_record(rng, 80, offset=64, p_amb=0)
            if k == 17:
                qual = qual[:40] + b"5" + qual[41:]
            f.write(b"@r%d\n%s\n+\n%s\n" % (k, seq, qual))
    ends = []
    for on in (False, True):
        cmd = [sys.executable, os.path.join(ROOT, "moira.py"), "-ffq", str(fq), "-fo", "64", "-c", "false", "--silent", "-op", str(tmp_path / ("o%d" % on))]
        p = subprocess.run(cmd + (["--device_pack"] if on else []), capture_output=True, text=True, cwd=ROOT, timeout=120)
        ends.append((p.returncode, [l for l in p.stderr.split("\n") if l.startswith("ValueError")]))
    assert ends[0] == ends[1] and ends[0][0] != 0 and ends[0][1] == ["ValueError: Qualities must have positive values."]
