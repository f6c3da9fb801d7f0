"""What of fasta+qual input on the device needs no device: the argument checks of mpb_fasta_qual_index_host and
mpb_filter_fasta_qual_host (made before the context is looked at), the prototypes against the header's declarations, the build
lists, the CLI's --device_fasta_qual switch, its eligibility and its sentence, what --device_format and --device_collapse make
of it, and the consumer's loop over the two carried tails on an engine that parses on the host.  The lane code on the host:
tests/test_fasta_qual_lane_model.py; the kernels: tests/test_gpu_fasta_qual.py; the runs: tests/test_gpu_fasta_qual_cli.py."""
import ctypes as C
import io
import os
import types

import numpy as np
import pytest

from helpers import fasta_qual_inputs as X
from moira_amd import _lib as L
from moira_amd import build as B
from moira_amd import cli
from moira_amd import fastio as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
FTEXT, QTEXT = X.render([(b"a", b"ACGT", [1, 2, 3, 4]), (b"b", b"GG", [40, 41])])
OUTS = ("n", "f_consumed", "q_consumed", "out_used", "why", "which", "bad_record")


def entry_call(filt, null=(), ftext=FTEXT, qtext=QTEXT, fbytes=None, qbytes=None, max_records=10, max_len=0, out_cap=64, rows=4):
    lib = L.load()
    out, idx = np.full(64, 7, np.uint8), np.full((4, 6), 7, np.int64)
    i64 = {k: C.c_int64(-7) for k in ("n", "f_consumed", "q_consumed", "out_used", "bad_record", "bad_pack")}
    i32 = {k: C.c_int32(-7) for k in ("why", "which")}
    ref = lambda k: None if k in null else C.byref(i64[k] if k in i64 else i32[k])
    a = [None, None if "ftext" in null else ftext, len(ftext) if fbytes is None else fbytes, None if "qtext" in null else qtext,
         len(qtext) if qbytes is None else qbytes, 1, max_records, max_len, None if "out" in null else out.ctypes.data, out_cap,
         None if "idx" in null else idx.ctypes.data, rows] + [ref(k) for k in OUTS]
    if not filt:
        rc = lib.mpb_fasta_qual_index_host(*a)
    else:
        res = [np.full(4, 7, t) for t in (np.float64, np.int32, np.uint8, np.int32, np.uint8)]
        params = L.FilterParams(0.005, 0.01, float("nan"), 0, 0)        # (maxerrors NaN: none)
        ptrs = [None if k in null else r.ctypes.data for k, r in zip(("ee", "ns", "pass", "len_out", "flags_out"), res)]
        rc = lib.mpb_filter_fasta_qual_host(*a, 0, None if "params" in null else C.byref(params), 0, *ptrs,
                                            None, None if "bad_pack" in null else C.byref(i64["bad_pack"]))
        assert all((r == 7).all() for r in res)
    assert (out == 7).all() and (idx == 7).all()             # nothing is written without a context
    return rc, lib.mpb_last_error().decode()


@pytest.mark.parametrize("filt", [False, True], ids=["index", "filter"])
def test_argument_errors_are_invalid_with_or_without_a_device(filt):
    rc, msg = entry_call(filt)
    assert rc == L.E_INVALID and "ctx is NULL" in msg        # good arguments: only the context is missing
    cases = [dict(null=("ftext",)), dict(null=("qtext",)), dict(null=("idx",))] + [dict(null=(k,)) for k in OUTS]
    cases += [dict(fbytes=-1), dict(qbytes=-1), dict(max_records=-1), dict(max_len=-1), dict(out_cap=-1), dict(rows=-1),
              dict(fbytes=(1 << 30) + 1), dict(qbytes=(1 << 30) + 1), dict(out_cap=(1 << 30) + 1)]
    cases += [dict(null=("ee",)), dict(null=("ns",)), dict(null=("pass",)), dict(null=("params",))] if filt else [dict(null=("out",))]
    for kw in cases:
        rc, msg = entry_call(filt, **kw)
        assert rc == L.E_INVALID and "ctx is NULL" not in msg, (kw, msg)
    assert "1 GiB" in entry_call(filt, qbytes=(1 << 30) + 1)[1] and "out_cap" in entry_call(filt, out_cap=(1 << 30) + 1)[1]
    # what is taken: no records asked for, empty texts (with or without a pointer), and in the filter entry no out, lengths or flags
    taken = [dict(max_records=0), dict(rows=0), dict(ftext=b"", qtext=b""), dict(fbytes=0, qbytes=0, null=("ftext", "qtext")), dict(out_cap=0),
             dict(max_len=1 << 30)]
    taken += [dict(null=("out",)), dict(null=("len_out", "flags_out", "bad_pack"))] if filt else []
    for kw in taken:
        assert "ctx is NULL" in entry_call(filt, **kw)[1], kw


def test_the_entries_are_declared_as_their_prototypes_say_and_the_unit_is_built():
    hdr = open(os.path.join(ROOT, "include", "moira_pb.h")).read()
    by_width = {"int64_t": C.c_int64, "int32_t": C.c_int32}
    for name, count in (("mpb_fasta_qual_index_host", 19), ("mpb_filter_fasta_qual_host", 29)):
        decl = hdr[hdr.index("int %s(" % name):].split(";")[0]
        proto = L.PROTOTYPES[name]
        assert proto[0] is C.c_int and len(proto[1]) == decl.count(",") + 1 == count
        for arg, ctype in zip(decl[decl.index("(") + 1:].rstrip(")").split(","), proto[1]):
            if "*" not in arg:
                assert ctype is by_width[arg.split()[0]], arg
            else:
                assert ctype not in by_width.values(), arg
    for k, v in (("NAMES", 5), ("EMPTY", 6), ("TOKEN", 7), ("LENGTH", 8), ("TRUNCATED", 9)):
        assert "#define MPB_FA_WHY_%s" % k in hdr and getattr(L, "FA_WHY_" + k) == v == getattr(X, k)
    assert L.FA_WHY[:5] == L.FQ_WHY and len(L.FA_WHY) == 10
    names = [os.path.basename(p) for p in B.SOURCES]
    assert "mpb_fasta_qual_kernels.hip" in names and "mpb_fasta_qual.cpp" in names
    assert "mpb_fasta_qual_lane.inc" in [os.path.basename(p) for p in B.DEPS]
    assert "#define MPB_K_COUNT     22" in hdr               # no timing id of its own: the kernels' header says where they are timed
    unit = open(os.path.join(ROOT, "moira_amd", "csrc", "mpb_fasta_qual_kernels.hip")).read()
    assert "MPB_K_FQ_ROWS" in unit and all(k in unit for k in ("k_fa_count", "k_fa_scan", "k_fa_write"))
    assert "mpb_fasta_qual_index_host, mpb_filter_fasta_qual_host and mpb_destroy" in hdr      # the calls that end a generation


# ---- the switch ------------------------------------------------------------------------------------------------------------------

def test_the_parser_knows_the_switch_and_it_goes_through_the_paths_owner():
    p = cli.build_parser()
    off, on = p.parse_args(["-ff", "a", "-fq", "b"]), p.parse_args(["-ff", "a", "-fq", "b", "--device_fasta_qual"])
    assert off.device_fasta_qual is False and on.device_fasta_qual is True
    text = " ".join(p.format_help().split())
    assert "--device_fasta_qual" in text and "it needs no other switch" in text and cli.DEVICE_FASTA_QUAL_MEASURED in text
    assert "Paired fasta+qual input stays on the host" in text
    # the two older switches say what they said
    assert "Paired input and fasta+qual input stay on the host indexer" in text and "Where it does not apply (fasta+qual input, the line parser" in text
    assert cli._DevicePaths().fasta_qual is False and cli._DevicePaths(("device_pack", "device_index")).fasta_qual is False
    said = []
    d = cli._DevicePaths({"device_fasta_qual"}, 0, said.append)
    assert d.fasta_qual and d.engine is None and not d.index and not d.pack
    d.fasta_qual_refused("quality token"), d.fasta_qual_refused("again")
    assert said == ["--device_fasta_qual: the device did not take a block (quality token): the host parser is used for it."]


def fake_backend(call=True, one_gpu=True, **engine):
    be = lambda *a, **k: None
    be.engine = types.SimpleNamespace(device=0, **engine)
    be.matrix = lambda *a, **k: None
    if call:
        be.engine.filter_fasta_qual = lambda *a, **k: None
    if one_gpu:
        be.text = be.text_choice = lambda *a, **k: {}
    return be


def test_eligibility():
    from test_cli_golden import reference_args
    fq = os.path.join(GOLD, "test1.fastq.gz")
    a = reference_args(paired=False, forward_fasta="x.fasta", forward_qual="x.qual")
    assert cli._device_fasta_qual_eligible(a, fake_backend())
    assert cli._device_fasta_qual_eligible(reference_args(paired=False, forward_fasta="x", forward_qual="y", collapse=False, truncate=100,
                                                          pipeline="USEARCH"), fake_backend())
    assert not cli._device_fasta_qual_eligible(a, fake_backend(call=False))
    assert not cli._device_fasta_qual_eligible(a, fake_backend(one_gpu=False))
    assert not cli._device_fasta_qual_eligible(reference_args(paired=False, forward_fastq=fq), fake_backend())
    assert not cli._device_fasta_qual_eligible(reference_args(paired=False, forward_fasta="x"), fake_backend())
    assert not cli._device_fasta_qual_eligible(reference_args(paired=True, forward_fasta="x", forward_qual="y", reverse_fasta="x", reverse_qual="y"),
                                               fake_backend())
    assert not cli._device_fasta_qual_eligible(reference_args(paired=False, forward_fasta="x", forward_qual="y", only_contig=True), fake_backend())
    # the FASTQ switches know nothing of it
    assert not cli._device_pack_eligible(a, fake_backend()) and not cli._device_index_eligible(a, fake_backend(filter_fastq=None))


def test_format_and_collapse_go_on_from_the_new_switch_and_from_the_old_pair_as_before():
    from test_cli_golden import reference_args
    be = fake_backend(format_text=None, collapse_text=None)
    plain = reference_args(paired=False, forward_fasta="x", forward_qual="y", collapse=False)
    coll = reference_args(paired=False, forward_fasta="x", forward_qual="y", collapse=True)
    for on, want in (({"device_fasta_qual"}, True), ({"device_index", "device_pack"}, True), ({"device_fasta_qual", "device_pack"}, True),
                     ({"device_index"}, False), ({"device_pack"}, False), (set(), False), ({"device_compress"}, False)):
        assert cli._device_format_eligible(plain, be, on) is want and cli._device_collapse_eligible(coll, be, on) is want, on
        assert not cli._device_format_eligible(coll, be, on) and not cli._device_collapse_eligible(plain, be, on)
    assert not cli._device_format_eligible(reference_args(paired=False, forward_fasta="x", forward_qual="y", collapse=False, pipeline="USEARCH"),
                                           be, {"device_fasta_qual"})
    assert not cli._device_format_eligible(plain, fake_backend(), {"device_fasta_qual"})
    assert not cli._device_collapse_eligible(coll, fake_backend(), {"device_fasta_qual"})


def test_the_switch_says_its_sentence_where_it_does_not_apply_and_the_output_is_unchanged(tmp_path, oracle):
    from test_cli_golden import oracle_backend, reference_args, same_files
    for name, kw, want in (("off", {}, []), ("on", dict(device_fasta_qual=True), ["--device_fasta_qual"]),
                           ("more", dict(device_fasta_qual=True, device_format=True, collapse=False), ["--device_fasta_qual", "--device_format"]),
                           ("quiet", dict(device_fasta_qual=True, nowarnings=True), [])):
        log = io.StringIO()
        a = reference_args(paired=False, forward_fastq=os.path.join(GOLD, "test1.fastq.gz"), output_prefix=str(tmp_path / name), **kw)
        assert cli.main(a, backend=oracle_backend(oracle), out=log) == 0
        lines = [l for l in log.getvalue().splitlines() if "does not apply to this run" in l]
        assert [l.split(" ")[0] for l in lines] == want
        if want:
            assert lines[0] == cli.DEVICE_FASTA_QUAL_SENTENCE
        if kw.get("collapse", True):
            same_files(str(tmp_path / name), "forward")
    # fasta+qual input on a backend without the call: the sentence, and the host parser's files
    from helpers import bgzf_inputs
    _, f, q = bgzf_inputs.golden_renderings()
    (tmp_path / "g.fasta").write_bytes(f), (tmp_path / "g.qual").write_bytes(q)
    log = io.StringIO()
    a = reference_args(paired=False, forward_fasta=str(tmp_path / "g.fasta"), forward_qual=str(tmp_path / "g.qual"),
                       output_prefix=str(tmp_path / "fa"), device_fasta_qual=True)
    assert cli.main(a, backend=oracle_backend(oracle), out=log) == 0
    assert log.getvalue().count(cli.DEVICE_FASTA_QUAL_SENTENCE) == 1
    same_files(str(tmp_path / "fa"), "forward")


# ---- the consumer's loop, on an engine that parses on the host ---------------------------------------------------------------------

class HostEngine:
    """filter_fasta_qual as the device entry behaves, made of fastio.fasta_qual_index: NotTaken where the host says Unsupported."""

    class NotTaken(Exception):
        pass

    def __init__(self, refuse=()):
        self.calls, self.refuse = [], refuse

    def filter_fasta_qual(self, fbuf, qbuf, final=True, max_records=None, **kw):
        self.calls.append((len(fbuf), len(qbuf), final))
        if (len(self.calls) - 1) % 3 in self.refuse:
            raise self.NotTaken("refused by the test")
        out, idx = np.empty(2 * len(fbuf) + 16, np.uint8), np.empty((min(max_records, len(fbuf) // 2 + 1), 6), np.int64)
        n, fc, qc, used = F.fasta_qual_index(fbuf, qbuf, final, len(idx), out, idx)
        return types.SimpleNamespace(text=out[:used], idx=idx[:n], f_consumed=fc, q_consumed=qc, ee=np.zeros(n), has_n=np.zeros(n, bool),
                                     resident=len(self.calls))


def records_of(chunks):
    out = []
    for buf, idx, aux, filtered in chunks:
        assert aux is None and len(idx) > 0
        buf = bytes(buf)
        out += [(buf[r[0]:r[0] + r[1]], buf[r[2]:r[2] + r[3]], buf[r[4]:r[4] + r[5]]) for r in idx.tolist()]
    return out


@pytest.mark.parametrize("blocks", [(1 << 20, 1 << 20), (700, 300), (64, 4096), (4096, 64), (1, 1)])
def test_the_consumer_carries_both_tails_and_reads_on_whichever_file_starves(blocks):
    recs = [(b"read%d" % i, (b"ACGTN" * 20)[:1 + (i * 7) % 90], [(i + j) % 255 for j in range(1 + (i * 7) % 90)]) for i in range(120)]
    f, q = X.render(recs, fhdr=b" x", last_eol=False)
    want = [(name, seq, bytes(quals)) for name, seq, quals in recs]
    for max_records, refuse in ((1000, ()), (7, ()), (50, (0, 2))):     # (refuse: the calls, counted modulo 3, that are handed back)
        eng, said = HostEngine(refuse), []
        streams = cli._DeferredFastaQualStreams((io.BytesIO(f), io.BytesIO(q)), blocks)
        consumer = cli._DeviceFastaQual(eng, {}, max_records, said.append, not_taken=HostEngine.NotTaken)
        try:
            chunks = list(consumer.run(streams))
        finally:
            streams.close()
        assert records_of(chunks) == want, (blocks, max_records)
        assert all(len(c[1]) <= max_records for c in chunks)
        came_back = [c for c in chunks if c[3] is None]
        assert len(said) == sum(k % 3 in refuse for k in range(len(eng.calls))) and (len(came_back) > 0) == bool(refuse)
        assert all(c[3].resident > 0 for c in chunks if c[3] is not None)
        assert eng.calls[-1][2] is True and (blocks[0] >= len(f) or len(eng.calls) > 2)


def test_texts_the_host_does_not_take_either_are_the_runs_to_take():
    f, q = X.render([(b"a", b"ACGT", [1, 2, 300, 4])])
    streams = cli._DeferredFastaQualStreams((io.BytesIO(f), io.BytesIO(q)), (1 << 20, 1 << 20))
    consumer = cli._DeviceFastaQual(HostEngine(), {}, 10, lambda e: None, not_taken=HostEngine.NotTaken)

    class Both(HostEngine):
        def filter_fasta_qual(self, *a, **k):
            try:
                return HostEngine.filter_fasta_qual(self, *a, **k)
            except F.Unsupported:
                raise self.NotTaken("quality token")
    consumer.engine = Both()
    try:
        with pytest.raises(F.Unsupported):
            list(consumer.run(streams))
    finally:
        streams.close()
