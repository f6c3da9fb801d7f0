"""CPU side of the device contig builder (include/moira_pb.h: mpb_pair_rows, mpb_contig_posterior_tables; the CLI's
--device_contigs where it does not apply).  mpb_pair_rows is the only place the offsets of a pair are trusted from; the tables
are what the device reads in `posterior` mode instead of calling pow.  The lane code: tests/test_contig_device_model.py; the
kernel: tests/test_gpu_contigs.py."""
import ctypes
import io
import os

import numpy as np
import pytest

from moira_amd import _lib as L
from moira_amd import cli
from moira_amd import contig as CT
from moira_amd import engine as E
from moira_amd import fastio as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def golden_chunk():
    """The golden paired input as the CLI's byte-level path sees it: one chunk of both files, indexed."""
    from moira_amd.cli import open_input_binary
    ffh, rfh = open_input_binary(os.path.join(GOLD, "test1.fastq.gz"), 1), open_input_binary(os.path.join(GOLD, "test2.fastq.bz2"), 1)
    try:
        chunks = list(F.PairedFastqChunks(ffh, rfh, 65536, threads=1))
    finally:
        ffh.close()
        rfh.close()
    assert len(chunks) == 1
    fbuf, fidx, rbuf, ridx = chunks[0]
    assert len(fidx) == len(ridx) == 1000
    return fbuf, np.ascontiguousarray(fidx), rbuf, np.ascontiguousarray(ridx)


def nbytes(buf):
    return int(buf.size) if isinstance(buf, np.ndarray) else len(buf)


def test_descriptor_layout():
    assert ctypes.sizeof(L.PairRow) == 56 == E.PAIR_ROW_DTYPE.itemsize and ctypes.sizeof(L.ContigParams) == 32
    assert [n for n, _ in L.PairRow._fields_] == list(E.PAIR_ROW_DTYPE.names)
    assert L.CONTIG_MAX_LEN == 384


def test_descriptors_of_the_golden_paired_chunk_equal_the_index_columns(golden_chunk):
    fbuf, fidx, rbuf, ridx = golden_chunk
    rec_cap = int((fidx[:, 1] + 2 * (fidx[:, 3] + ridx[:, 3])).max()) + 8
    rows = E.pair_rows(fidx, ridx, nbytes(fbuf), nbytes(rbuf), rec_cap)
    assert np.array_equal(rows["fhdr_off"], fidx[:, F.HDR_OFF]) and np.array_equal(rows["hdr_len"], fidx[:, F.HDR_LEN])
    assert np.array_equal(rows["fseq_off"], fidx[:, F.SEQ_OFF]) and np.array_equal(rows["fqual_off"], fidx[:, F.QUAL_OFF])
    assert np.array_equal(rows["rseq_off"], ridx[:, F.SEQ_OFF]) and np.array_equal(rows["rqual_off"], ridx[:, F.QUAL_OFF])
    assert np.array_equal(rows["l1"], fidx[:, F.SEQ_LEN]) and np.array_equal(rows["l2"], ridx[:, F.SEQ_LEN]) and not rows["pad"].any()
    # a record that ends exactly at the end of its text, and the tightest rec_cap, are fine
    tight = int((fidx[:, 1] + 2 * (fidx[:, 3] + ridx[:, 3])).max())
    last = int(max((fidx[:, F.QUAL_OFF] + fidx[:, F.QUAL_LEN]).max(), (fidx[:, F.HDR_OFF] + fidx[:, F.HDR_LEN]).max()))
    E.pair_rows(fidx, ridx, last, nbytes(rbuf), tight)
    assert len(E.pair_rows(fidx[:0], ridx[:0], 0, 0, 8)) == 0


def test_every_refusal_reports_its_pair(golden_chunk):
    fbuf, fidx, rbuf, ridx = golden_chunk
    nf, nr = nbytes(fbuf), nbytes(rbuf)
    rec_cap = int((fidx[:, 1] + 2 * (fidx[:, 3] + ridx[:, 3])).max()) + 8

    def refused(at, which, col, value, rec_cap=rec_cap, nf=nf, nr=nr):
        f, r = fidx.copy(), ridx.copy()
        (f if which == "f" else r)[at, col] = value
        with pytest.raises(ValueError) as e:
            E.pair_rows(f, r, nf, nr, rec_cap)
        assert e.value.bad_record == at, (at, which, col, value, str(e.value))
        return str(e.value)

    assert "negative" in refused(3, "f", F.SEQ_OFF, -1)
    assert "negative" in refused(5, "r", F.QUAL_OFF, -7)
    assert "negative" in refused(6, "f", F.HDR_OFF, -1)
    assert "negative" in refused(7, "f", F.HDR_LEN, -2)
    assert "past the text" in refused(11, "f", F.SEQ_OFF, nf - int(fidx[11, F.SEQ_LEN]) + 1)
    assert "past the text" in refused(12, "f", F.QUAL_OFF, nf)
    assert "past the text" in refused(13, "r", F.SEQ_OFF, nr - int(ridx[13, F.SEQ_LEN]) + 1)
    assert "past the text" in refused(14, "r", F.QUAL_OFF, 1 << 40)
    assert "past the text" in refused(15, "f", F.HDR_OFF, nf - int(fidx[15, F.HDR_LEN]) + 1)
    assert "differ in length" in refused(21, "f", F.QUAL_LEN, int(fidx[21, F.SEQ_LEN]) - 1)
    assert "differ in length" in refused(22, "r", F.SEQ_LEN, int(ridx[22, F.SEQ_LEN]) + 1)
    assert "negative" in refused(23, "r", F.SEQ_LEN, -1)
    assert "2^31" in refused(24, "f", F.SEQ_LEN, 1 << 31)
    # hdr_len + 2 (l1 + l2) > rec_cap: the first pair that does not fit a slot one byte too small for the largest
    need = fidx[:, 1] + 2 * (fidx[:, 3] + ridx[:, 3])
    first = int(np.argmax(need == need.max()))
    with pytest.raises(ValueError) as e:
        E.pair_rows(fidx, ridx, nf, nr, int(need.max()) - 1)
    assert e.value.bad_record == first and "rec_cap" in str(e.value)
    # the first bad pair wins
    f = fidx.copy()
    f[40, F.SEQ_OFF] = -1
    f[30, F.QUAL_OFF] = nf
    with pytest.raises(ValueError) as e:
        E.pair_rows(f, ridx, nf, nr, rec_cap)
    assert e.value.bad_record == 30
    # lengths the device does not take are no errors here: they are handed back
    f, r = fidx.copy(), ridx.copy()
    f[2, F.SEQ_LEN] = f[2, F.QUAL_LEN] = 0
    rows = E.pair_rows(f, r, nf, nr, rec_cap)
    assert rows["l1"][2] == 0


def test_posterior_tables_equal_make_contig_on_one_column_alignments():
    """Every (q1, q2) in 0..93 squared, both tables: a one-column alignment of two equal bases (match) and of two different ones
    (mismatch), through the host library's make_contig -- the expressions and the libm the tables were built with."""
    t = np.empty((2, 256, 256), np.int32)
    assert L.load().mpb_contig_posterior_tables(t[0].ctypes.data, t[1].ctypes.data) == 0
    assert L.load().mpb_contig_posterior_tables(None, t[1].ctypes.data) == L.E_INVALID
    for q1 in range(94):
        for q2 in range(94):
            contig, cq, ov, gaps, mism = CT.make_contig("A", [q1], "A", [q2], 20, 6, "posterior", 0, False)
            assert (contig, cq, mism) == ("A", [int(t[0, q1, q2])], 0), (q1, q2)
            contig, cq, ov, gaps, mism = CT.make_contig("A", [q1], "C", [q2], 20, 6, "posterior", 0, False)
            want = ("N", [2]) if q1 == q2 else ("A" if q1 > q2 else "C", [int(t[1, q1, q2])])
            assert (contig, cq, mism) == want + (1,), (q1, q2)
    assert (t[:, :94, :94] > np.iinfo(np.int32).min).all()             # (INT32_MIN marks an entry that is no finite integer)


def test_device_contigs_parses_and_is_off_by_default():
    base = ["-ffq", "a.fastq", "-rfq", "b.fastq", "--paired"]
    off, on = cli.parse_arguments(base), cli.parse_arguments(base + ["--device_contigs"])
    assert off.device_contigs is False and on.device_contigs is True
    d_off, d_on = dict(vars(off)), dict(vars(on))
    d_off.pop("device_contigs"), d_on.pop("device_contigs")
    assert d_off == d_on and d_off["device_pack"] is False
    assert "--device_contigs" in cli.build_parser().format_help()


def test_device_contigs_on_a_cpu_backend_says_so_once_and_changes_nothing(tmp_path, oracle):
    from test_cli_golden import oracle_backend, reference_args, same_files
    said = []
    for name, on in (("off", False), ("on", True)):
        out, msg = str(tmp_path / name), io.StringIO()
        a = reference_args(paired=True, forward_fastq=os.path.join(GOLD, "test1.fastq.gz"), output_prefix=out,
                           reverse_fastq=os.path.join(GOLD, "test2.fastq.bz2"))
        if on:
            a.device_contigs = True
        assert cli.main(a, backend=oracle_backend(oracle), out=msg) == 0
        said.append([l for l in msg.getvalue().split("\n") if "device_contigs" in l])
        same_files(out, "paired")
    assert said[0] == [] and len(said[1]) == 1 and "the host aligner is used" in said[1][0]


def test_contigs_from_fastq_without_an_engine_is_untouched(golden_chunk):
    """engine=None is the default and the old code path: same bytes as before for the golden chunk's first pairs, against the
    per-pair functions."""
    fbuf, fidx, rbuf, ridx = golden_chunk
    cbuf, cidx, aux = CT.contigs_from_fastq(fbuf, fidx[:20], rbuf, ridx[:20], threads=2)
    fb, rb = bytes(fbuf), bytes(rbuf)
    for i in range(20):
        seq = lambda b, r: b[r[F.SEQ_OFF]:r[F.SEQ_OFF] + r[F.SEQ_LEN]].decode()
        qual = lambda b, r: [c - 33 for c in b[r[F.QUAL_OFF]:r[F.QUAL_OFF] + r[F.QUAL_LEN]]]
        rs, rq = CT.reverse_complement(seq(rb, ridx[i]), qual(rb, ridx[i]))
        a1, a2, _ = CT.nw_align(seq(fb, fidx[i]), rs, 1, -1, -2)
        contig, cq, ov, gaps, mism = CT.make_contig(a1, qual(fb, fidx[i]), a2, rq, 20, 6, "best", 40, False)
        b = bytes(cbuf)
        assert b[cidx[i, 2]:cidx[i, 2] + cidx[i, 3]].decode() == contig and [c - 33 for c in b[cidx[i, 4]:cidx[i, 4] + cidx[i, 5]]] == cq
        assert tuple(aux[i]) == (ov, gaps, mism)
