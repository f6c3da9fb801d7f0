"""What of the text-alone paired entry needs no device: the argument checks of mpb_contigs_filter_fastq_host (made before the
context is looked at), the CLI's --device_pair_index switch and its eligibility, and the consumer's side of the switch
(cli._DevicePairIndexer) against fastio.PairedFastqChunks with a fake engine whose contigs_filter_fastq is fastio.index x 2 +
fastio.first_header_mismatch, every pair handed back to the host aligner.  The lane code on the host:
tests/test_pair_lane_model.py; the kernels: tests/test_gpu_pair_index.py."""
import ctypes as C
import io
import os
import re
import types

import numpy as np
import pytest

from helpers import contig_pairs as P
from helpers import pair_index_inputs as X
from moira_amd import _lib as L
from moira_amd import cli
from moira_amd import contig as CT
from moira_amd import engine as E
from moira_amd import fastio as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
TEXT = b"@r\nACGT\n+\nIIII\n"
OUT_PTRS = ("n_f", "f_bad_kind", "n_r", "r_bad_kind", "n_pairs", "mismatch", "n_built", "f_consumed", "r_consumed", "why", "which", "rec_cap")
ARRAYS = ("fidx", "ridx", "out_buf", "out_idx", "overlap", "gaps", "mismatches", "done", "ee", "ns", "pass", "filtered")


# ---- the C ABI's argument checks ---------------------------------------------------------------------------------------------

def entry_call(null=(), ftext=TEXT, rtext=TEXT, fbytes=None, rbytes=None, max_records=10, offset=33, prm=(1, -1, -2, 20, 6, 0, 40, 0),
               cap=4, out_cap=4096, max_len=0, fparams=E.Engine.params()):
    lib = L.load()
    a = {k: np.zeros(4096, np.uint8) for k in ARRAYS}
    i64, i32 = {k: C.c_int64(-7) for k in OUT_PTRS}, {k: C.c_int32(-7) for k in OUT_PTRS}
    arr = lambda k: None if k in null else a[k].ctypes.data
    p64 = lambda k: None if k in null else C.byref(i64[k])
    p32 = lambda k: None if k in null else C.byref(i32[k])
    cp = L.ContigParams(*prm) if prm is not None else None
    counts, frc, fbad = L.FilterCounts(), C.c_int(-7), C.c_int64(5)
    rc = lib.mpb_contigs_filter_fastq_host(
        None, None if "ftext" in null else ftext, len(ftext) if fbytes is None else fbytes, 1,
        None if "rtext" in null else rtext, len(rtext) if rbytes is None else rbytes, 1, max_records, offset,
        C.byref(cp) if cp is not None else None, arr("fidx"), arr("ridx"), cap, p64("n_f"), p32("f_bad_kind"), p64("n_r"), p32("r_bad_kind"),
        p64("n_pairs"), p64("mismatch"), p64("n_built"), p64("f_consumed"), p64("r_consumed"), p32("why"), p32("which"), p64("rec_cap"),
        arr("out_buf"), out_cap, arr("out_idx"), arr("overlap"), arr("gaps"), arr("mismatches"), arr("done"), None, None,
        max_len, 0, C.byref(fparams) if fparams is not None else None, 0, arr("ee"), arr("ns"), arr("pass"), None, None, arr("filtered"),
        C.byref(counts), C.byref(frc), C.byref(fbad))
    return rc, lib.mpb_last_error().decode(), (frc.value, fbad.value)


def test_argument_errors_are_invalid_with_or_without_a_device():
    rc, msg, f = entry_call()
    assert rc == L.E_INVALID and "ctx is NULL" in msg and f == (0, -1)      # good arguments: only the context is missing
    bad = [dict(null=("ftext",)), dict(null=("rtext",)), dict(fbytes=-1), dict(rbytes=-1), dict(max_records=-1), dict(max_len=-1), dict(cap=0),
           dict(out_cap=-1), dict(null=("fidx",)), dict(null=("ridx",))] + [dict(null=(k,)) for k in OUT_PTRS]
    for kw in bad:
        rc, msg, _ = entry_call(**kw)
        assert rc == L.E_INVALID and "mpb_contigs_filter_fastq_host: bad arguments" in msg, kw
    for k in ARRAYS[2:]:
        rc, msg, _ = entry_call(null=(k,))
        assert rc == L.E_INVALID and "NULL host buffer" in msg, k
    for kw in (dict(fbytes=(1 << 30) + 1), dict(rbytes=(1 << 30) + 1)):
        rc, msg, _ = entry_call(**kw)
        assert rc == L.E_INVALID and "at most 1073741824 bytes (1 GiB) of text" in msg
    assert "ctx is NULL" in entry_call(ftext=b"", rtext=b"", null=("ftext", "rtext"))[1]        # an empty text needs no pointer


def test_parameter_errors_come_with_todays_messages():
    assert "params is NULL" in entry_call(prm=None)[1]
    for prm, what in (((1, -1, -2, 0, 6, 0, 40, 0), "insert must be a positive integer"), ((1, -1, -2, 20, 0, 0, 40, 0), "deltaq must be a positive integer"),
                      ((1, -1, -2, 20, 6, 0, -1, 0), "qscore_cap must be a non-negative integer"), ((1, -1, -2, 20, 6, 3, 40, 0), "consensus_qscore must be")):
        rc, msg, _ = entry_call(prm=prm)
        assert rc == L.E_INVALID and what in msg
    assert "params is NULL" in entry_call(fparams=None)[1]
    assert "Alpha must be between 0 and 1" in entry_call(fparams=L.FilterParams(2.0, 0.01, float("nan"), 0, 0))[1]


def test_the_entry_is_declared_and_the_pinned_tables_keep_their_length():
    hdr = open(os.path.join(ROOT, "include", "moira_pb.h")).read()
    declared = set(re.findall(r"^(?:int|const char \*|void) \*?(mpb_\w+)\(", hdr, re.M))
    assert "mpb_contigs_filter_fastq_host" in declared and declared <= set(L.PROTOTYPES)       # the ctypes table covers the header
    assert len(L.PROTOTYPES["mpb_contigs_filter_fastq_host"][1]) == hdr[hdr.index("int mpb_contigs_filter_fastq_host("):].split(";")[0].count(",") + 1
    assert "#define MPB_K_COUNT     22" in hdr and len(L.FQ_WHY) == 5
    assert len(re.findall(r"#define MPB_FQ_WHY_\w+ +\d", hdr)) == 5
    kernels = list(L.KERNEL_NAMES) + list(L.CONTIG_KERNEL_NAMES) + list(L.BGZF_KERNEL_NAMES) + list(L.INFLATE_KERNEL_NAMES) + list(L.INDEX_KERNEL_NAMES)
    assert sorted(kernels) == list(range(22))
    assert "MPB_K_CONTIG_ROWS" in hdr[hdr.index("The chunk call with the filter behind it from the two mates"):hdr.index("int mpb_contigs_filter_fastq_host(")]


# ---- the switch ------------------------------------------------------------------------------------------------------------------

def test_the_parser_knows_the_switch_and_it_is_off_by_default():
    p = cli.build_parser()
    base = ["-ffq", "a", "-rfq", "b", "--paired"]
    off, on = p.parse_args(base), p.parse_args(base + ["--device_pair_index"])
    assert off.device_pair_index is False and on.device_pair_index is True
    d_off, d_on = dict(vars(off)), dict(vars(on))
    d_off.pop("device_pair_index"), d_on.pop("device_pair_index")
    assert d_off == d_on
    assert "--device_pair_index" in p.format_help()


def test_the_table_keeps_its_five_rows_and_the_paths_get_one_more_attribute():
    assert [r[0] for r in cli._DEVICE_PATHS] == ["device_pack", "device_contigs", "device_index", "device_compress", "device_inflate"]
    assert cli._DevicePaths().pair_index is False and cli._DevicePaths(("device_pack", "device_contigs")).pair_index is False
    said = []
    d = cli._DevicePaths({"device_pack", "device_contigs", "device_pair_index"}, 0, said.append)
    assert d.pair_index and d.pack and d.contigs and not d.index and d.engine is None
    e = E.NotTaken(1)
    e.which = 1
    d.pair_index_refused(e), d.pair_index_refused(E.NotTaken(2))
    assert len(said) == 1 and said[0].startswith("--device_pair_index: the device did not take a pair of blocks (")


def fake_backend(text=True, call=True):
    be = lambda *a, **k: None
    be.matrix = lambda *a, **k: None
    be.methods = ("poisson_binomial", "poisson")
    be.engine = types.SimpleNamespace(device=0, contigs_text=None, contigs_filter_text=None)
    if call:
        be.engine.contigs_filter_fastq = lambda *a, **k: None
    if text:
        be.text = lambda *a, **k: None
        be.text_choice = lambda *a, **k: {}
    return be


def test_eligibility():
    from test_cli_golden import reference_args
    fq = os.path.join(GOLD, "test1.fastq.gz")
    both = {"device_contigs", "device_pack"}
    paired = reference_args(paired=True, forward_fastq=fq, reverse_fastq=fq)
    assert cli._device_pair_index_eligible(paired, fake_backend(), both)
    assert not cli._device_pair_index_eligible(paired, fake_backend(), {"device_contigs"})
    assert not cli._device_pair_index_eligible(paired, fake_backend(), {"device_pack"})
    assert not cli._device_pair_index_eligible(paired, fake_backend(call=False), both)
    assert not cli._device_pair_index_eligible(paired, fake_backend(text=False), both)             # several GPUs: no text entry
    assert not cli._device_pair_index_eligible(reference_args(paired=False, forward_fastq=fq), fake_backend(), both)
    assert not cli._device_pair_index_eligible(reference_args(paired=True, forward_fasta="a", forward_qual="b", reverse_fasta="c", reverse_qual="d"),
                                               fake_backend(), both)
    assert not cli._device_pair_index_eligible(reference_args(paired=True, forward_fastq=fq, reverse_fastq=fq, only_contig=True), fake_backend(), both)
    assert not cli._device_index_eligible(paired, fake_backend())                                  # (pinned: --device_index stays single-end)


def test_the_switch_without_a_gpu_or_without_its_two_switches_says_so_once_and_changes_no_file(tmp_path, oracle):
    from test_cli_golden import oracle_backend, reference_args, same_files
    for name, kw, want in (("off", {}, []), ("on", dict(device_pair_index=True), ["--device_pair_index"]),
                           ("all", dict(device_pair_index=True, device_contigs=True, device_pack=True),
                            ["--device_pack", "--device_contigs", "--device_pair_index"]),
                           ("quiet", dict(device_pair_index=True, nowarnings=True), [])):
        log = io.StringIO()
        a = reference_args(paired=True, forward_fastq=os.path.join(GOLD, "test1.fastq.gz"), reverse_fastq=os.path.join(GOLD, "test2.fastq.bz2"),
                           output_prefix=str(tmp_path / name), **kw)
        assert cli.main(a, backend=oracle_backend(oracle), out=log) == 0
        lines = [l for l in log.getvalue().splitlines() if "does not apply to this run" in l]
        assert [l.split(" ")[0] for l in lines] == want
        if want:
            assert lines[-1] == cli.DEVICE_PAIR_INDEX_SENTENCE
        same_files(str(tmp_path / name), "paired")


# ---- the consumer's side, against fastio.PairedFastqChunks ---------------------------------------------------------------------------

class FakeEngine:
    """contigs_filter_fastq = fastio.index x 2 + fastio.first_header_mismatch; every pair is handed back (done all False, nothing
    filtered), so the host aligner builds the contigs through the merge the real call shares."""

    def __init__(self, refuse=(), fail=()):
        self.calls, self.refuse, self.fail = 0, set(refuse), set(fail)

    def contigs_filter_fastq(self, fbuf, rbuf, ffinal, rfinal, max_records, *a, **kw):
        k, self.calls = self.calls, self.calls + 1
        if k in self.refuse:
            e = E.NotTaken(2)
            e.which = 1
            raise e
        if k in self.fail:
            raise ValueError("refused for the test")
        f, r = F.index(fbuf, ffinal, max_records), F.index(rbuf, rfinal, max_records)
        n = min(len(f[0]), len(r[0]))
        mis = F.first_header_mismatch(fbuf, f[0][:n], rbuf, r[0][:n]) if n else -1
        nb = n if mis < 0 else mis
        rec_cap = int((f[0][:nb, 1] + 2 * (f[0][:nb, 3] + r[0][:nb, 3])).max()) + 8 if nb else 8
        cons = [F.index(b, fin, n)[1] if n else 0 for b, fin in ((fbuf, ffinal), (rbuf, rfinal))]
        return types.SimpleNamespace(
            fidx=f[0], ridx=r[0], f_bad=f[2], r_bad=r[2], f_consumed=cons[0], r_consumed=cons[1], mismatch=mis, n_pairs=n, n_built=nb,
            rec_cap=rec_cap, cbuf=np.zeros(nb * rec_cap, np.uint8), cidx=np.zeros((nb, 6), np.int64), aux=np.zeros((nb, 3), np.int32),
            done=np.zeros(nb, bool), ee=np.zeros(nb), has_n=np.zeros(nb, bool), filtered=np.zeros(nb, bool), filter_error=None)


def blocks_of(text, size):
    return iter([cli._DeferredBlock(text[a:a + size], False) for a in range(0, len(text), size)] + [cli._DeferredBlock(b"", True)])


def host_fused(fbuf, fidx, rbuf, ridx):
    cbuf, cidx, aux = CT.contigs_from_fastq(fbuf, fidx, rbuf, ridx, threads=2)
    return cbuf, cidx, aux, np.full(len(cidx), 2.0), np.zeros(len(cidx), bool), None


def signature(e):
    if e is None:
        return None
    if isinstance(e, F.PairedRecordError):
        return ("record", e.which, e.err.kind, e.err.header, getattr(e.err, "forward_header", None))
    return (type(e).__name__,) + tuple(e.args)


def drive(ftext, rtext, sizes, max_records=1000, engine=None, said=None):
    """-> ([records of a chunk], the exception the run ended with or None, the engine)."""
    engine = engine or FakeEngine()
    stub = lambda buf, idx, sel: (np.full(len(sel), 1.0), np.zeros(len(sel), bool))
    device = lambda f, r, ff, rf, mr: CT.contigs_from_fastq_text_filtered(f, r, ff, rf, mr, threads=2, engine=engine, backend_text=stub)
    refused = cli._SaidOnce((said if said is not None else []).append, "refused: %s")
    ix = cli._DevicePairIndexer(device, host_fused, max_records, refused, not_taken=E.NotTaken)
    streams = types.SimpleNamespace(blocks=[blocks_of(ftext, sizes[0]), blocks_of(rtext, sizes[1])], block=max(sizes))
    got, err = [], None
    try:
        for cbuf, cidx, aux, ee, has_n, ferr in ix.run(streams):
            assert ferr is None and len(ee) == len(cidx) == len(aux)
            got.append(P.records(cbuf, cidx))
    except (F.PairedRecordError, cli.NameMismatchError) as e:
        err = e
    return got, err, engine


def expect(ftext, rtext, block, max_records=1000):
    """fastio.PairedFastqChunks with what cli._fast_chunks does with its chunks."""
    out, err = [], None
    try:
        for fbuf, fidx, rbuf, ridx in F.PairedFastqChunks(io.BytesIO(ftext), io.BytesIO(rtext), max_records, block_bytes=block):
            bad = F.first_header_mismatch(fbuf, fidx, rbuf, ridx)
            n = len(fidx) if bad < 0 else bad
            if n:
                out.append(P.records(*CT.contigs_from_fastq(fbuf, fidx[:n], rbuf, ridx[:n], threads=2)[:2]))
            if bad >= 0:
                raise cli.NameMismatchError(F.header_of(fbuf, fidx[bad]), None, F.header_of(rbuf, ridx[bad]), None)
    except (F.PairedRecordError, cli.NameMismatchError) as e:
        err = e
    return out, err


LINE_ARGS = types.SimpleNamespace(forward_fastq="forward.fastq", reverse_fastq="reverse.fastq")


def line_parser(ftext, rtext):
    """The line parser over the same two texts -- it shares no code with the pairing loop -> (the headers of the pairs it yields
    before the end, the exception it ends with or None)."""
    files = [io.StringIO(t.decode("ascii"), newline=None) for t in (ftext, rtext)]
    files[0].moira_name, files[1].moira_name = LINE_ARGS.forward_fastq, LINE_ARGS.reverse_fastq
    headers, err = [], None
    try:
        for rec in cli.parse_fastq(files[0], files[1], 33, raw=True):
            headers.append(rec[0])
    except (cli.NameMismatchError, cli.EmptySeqError, cli.EmptyQualError, cli.LengthMismatchError) as e:
        err = e
    return headers, err


def as_the_run_raises(err):
    """(class, arguments) of what the run raises for the way the loop ended: a PairedRecordError goes through cli._record_error."""
    if isinstance(err, F.PairedRecordError):
        err = cli._record_error(err.which, err.err, LINE_ARGS)
    return None if err is None else (type(err), err.args)


def same(ftext, rtext, size, max_records=1000, **kw):
    got, err, eng = drive(ftext, rtext, (size, size), max_records, **kw)
    want, want_err = expect(ftext, rtext, size, max_records)
    assert got == want and signature(err) == signature(want_err)
    # both of those run fastio.paired_lockstep: the line parser is the witness that does not
    line_headers, line_err = line_parser(ftext, rtext)
    assert [h.decode("ascii").replace(":", "_") for c in got for h, _, _ in c] == line_headers      # (fastio.header_of's rule)
    assert as_the_run_raises(err) == as_the_run_raises(line_err)
    return got, err, eng


def small_pairs(n=60, seed=8):
    rng = np.random.default_rng(seed)
    return [P.make_pair(rng, int(rng.integers(20, 60)), int(rng.integers(20, 60)), "overlap") for _ in range(n)]


@pytest.mark.parametrize("size", (1000, 4096, 65536))
def test_the_golden_files_cut_into_blocks(size):
    f, r = X.golden_texts()
    got, err, _ = same(f, r, size, max_records=192)
    assert err is None and sum(len(c) for c in got) == 1000


def test_different_block_sizes_per_file():
    """(PairedFastqChunks has one block size: the chunk borders may differ, the pairs in order and the end may not)"""
    f, r = X.golden_texts()
    got, err, _ = drive(f, r, (1000, 7777), max_records=192)
    want, want_err = expect(f, r, 4096, 192)
    assert err is None and want_err is None and [x for c in got for x in c] == [x for c in want for x in c]


@pytest.mark.parametrize("longer", (0, 1))
def test_one_file_five_records_longer(longer):
    pairs = small_pairs()
    f, r = X.pair_texts(pairs)
    cut = X.pair_texts(pairs[:55])[1 - longer]
    f, r = (f, cut) if longer == 0 else (cut, r)
    for size in (300, 1 << 20):
        got, err, _ = same(f, r, size)
        assert err is None and sum(len(c) for c in got) == 55


@pytest.mark.parametrize("kind", (F.REC_EMPTY_SEQ, F.REC_EMPTY_QUAL, F.REC_LENGTH_MISMATCH))
@pytest.mark.parametrize("where", ("forward", "reverse", "both"))
def test_a_bad_record(kind, where):
    pairs = small_pairs()
    recs = [[(("p%d" % i).encode(), p.fwd.encode(), p.fq) for i, p in enumerate(pairs)],
            [(("p%d" % i).encode(), p.rev.encode(), p.rq) for i, p in enumerate(pairs)]]
    for which in {"forward": (0,), "reverse": (1,), "both": (0, 1)}[where]:
        name, seq, qual = recs[which][40]
        recs[which][40] = (name, b"" if kind == F.REC_EMPTY_SEQ else seq, b"" if kind == F.REC_EMPTY_QUAL else qual[:-1] if kind == F.REC_LENGTH_MISMATCH else qual)
    f, r = X.fastq_text(recs[0]), X.fastq_text(recs[1])
    for size in (300, 1 << 20):
        got, err, _ = same(f, r, size)
        assert isinstance(err, F.PairedRecordError) and err.err.kind == kind and err.which == (1 if where == "reverse" else 0)
        assert sum(len(c) for c in got) == 40
        if where == "reverse":
            assert err.err.forward_header == "p40"
    # the record error of pair n is raised only when both files hold record n: the other file ends first
    f_short = X.fastq_text(recs[0][:40]) if where == "reverse" else f
    r_short = X.fastq_text(recs[1][:40]) if where == "forward" else r
    if where != "both":
        got, err, _ = same(f_short, r_short, 300)
        assert err is None and sum(len(c) for c in got) == 40


@pytest.mark.parametrize("at", (0, 30, 59))
def test_a_header_mismatch_yields_the_pairs_before_it(at):
    pairs = small_pairs()
    names = [("p%d" % i).encode() for i in range(60)]
    rnames = list(names)
    rnames[at] = b"q%d" % at
    f, r = X.pair_texts(pairs, names, rnames)
    for size in (300, 1 << 20):
        got, err, _ = same(f, r, size)
        assert isinstance(err, cli.NameMismatchError) and sum(len(c) for c in got) == at


def test_crlf_files():
    f, r = X.pair_texts(small_pairs(), eol=b"\r\n")
    for size in (301, 1 << 20):
        got, err, _ = same(f, r, size)
        assert err is None and sum(len(c) for c in got) == 60


def test_a_handed_back_pair_of_blocks_goes_through_the_host_and_is_said_once():
    f, r = X.pair_texts(small_pairs())
    said = []
    got, err, eng = same(f, r, 700, engine=FakeEngine(refuse={1, 3}, fail={2}), said=said)
    assert err is None and eng.calls > 4 and said == ["refused: lone carriage return"]


def test_what_the_host_calls_unsupported_is_the_runs_to_take():
    f, r = X.pair_texts(small_pairs(5))
    with pytest.raises(F.Unsupported):
        drive(f, r[:30] + b"\rX" + r[32:], (1 << 20, 1 << 20), engine=FakeEngine(refuse={0}))
