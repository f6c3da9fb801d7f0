"""What of mpb_format_records_host and the contig generation needs no device: the entry's argument checks (made before the context
is looked at) with its ee and row validation, the prototype against the header, the old entry's refusal of kind 4, the
eligibility of --device_format and --device_collapse (paired with --device_pair_index, USEARCH single-end) with the sentences,
and the CLI's consumer side with an engine made of the host functions: a paired chunk that carries a generation has its records
AND its report lines formatted through the engine, one without goes the host way, said once.  The lane code on the host:
tests/test_format_records_model.py; the kernels: tests/test_gpu_format_records.py."""
import ctypes as C
import io
import os
import types

import numpy as np
import pytest

from helpers import format_inputs as X
from helpers import format_records_inputs as R
from moira_amd import _lib as L
from moira_amd import cli
from moira_amd import contig as CT
from moira_amd import engine as E
from moira_amd import fastio as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
TEXT, IDX = X.count_text(6, 3)
AUX = np.arange(18, dtype=np.int32).reshape(6, 3)


def entry_call(null=(), text=TEXT, idx=IDX, text_bytes=None, n_records=None, resident=0, sel=None, nsel=None, kind=4, relabel=None,
               relabel_index=None, labels=None, label_id=None, ee=None, aux=AUX, bgzf=0, out_cap=1 << 16, entry="mpb_format_records_host"):
    lib = L.load()
    out = np.zeros(1 << 16, np.uint8)
    got, needed, bad = C.c_int64(-7), C.c_int64(-7), C.c_int64(-7)
    idx = None if idx is None else np.ascontiguousarray(idx, np.int64)
    keep = [np.ascontiguousarray(a, t) if a is not None else None
            for a, t in ((sel, np.int64), (relabel_index, np.int64), (label_id, np.int32), (ee, np.float64), (aux, np.int32))]
    ptr = lambda a: None if a is None else a.ctypes.data
    enc = [s.encode() for s in labels or []]
    lab = (C.c_char_p * max(len(enc), 1))(*enc)
    head = (None, None if "text" in null else text, len(text or b"") if text_bytes is None else text_bytes, None if "idx" in null else ptr(idx),
            (0 if idx is None else len(idx)) if n_records is None else n_records, resident, ptr(keep[0]),
            (len(sel) if sel is not None else 0 if idx is None else len(idx)) if nsel is None else nsel, kind, 33, 33, 1, 0, relabel,
            ptr(keep[1]), C.cast(lab, C.c_void_p) if labels is not None else None, len(enc), ptr(keep[2]))
    tail = (bgzf, None if "out" in null else out.ctypes.data, out_cap, None if "out_bytes" in null else C.byref(got),
            None if "text_needed" in null else C.byref(needed), None if "bad_record" in null else C.byref(bad), None)
    mid = (ptr(keep[3]), ptr(keep[4])) if entry == "mpb_format_records_host" else ()
    rc = getattr(lib, entry)(*(head + mid + tail))
    return rc, lib.mpb_last_error().decode(), bad.value


def test_argument_errors_are_invalid_with_or_without_a_device():
    rc, msg, bad = entry_call()
    assert rc == L.E_INVALID and "ctx is NULL" in msg and bad == -1          # good arguments: only the context is missing
    cases = [(dict(null=("idx",)), "either text and idx"), (dict(null=("out_bytes",)), "bad arguments"), (dict(nsel=-1), "bad arguments"),
             (dict(kind=3), "kind 3"), (dict(kind=5), "kind 5"), (dict(kind=-1), "kind -1"),
             (dict(aux=None), "needs aux"), (dict(kind=2, aux=AUX), "aux goes with kind 4 alone"),
             (dict(labels=["a"], label_id=np.zeros(6)), "takes no labels"), (dict(labels=["a"]), "takes no labels"),
             (dict(relabel=b"S"), "relabel without relabel_index"),
             (dict(resident=3), "not both or neither"), (dict(resident=-1, null=("text", "idx"), idx=None), "is no generation"),
             (dict(resident=2, null=("text", "idx"), idx=None, n_records=6, nsel=6), "aux with a generation")]
    for kw, what in cases:
        rc, msg, _ = entry_call(**kw)
        assert rc == L.E_INVALID and "ctx is NULL" not in msg and "mpb_format_records_host: " in msg and what in msg, (kw, msg)
        assert "is not resident" not in msg
    # what is taken: every kind with ee, the resident form of a report without aux, no record at all
    for kw in (dict(ee=R.EE[:6]), dict(kind=0, aux=None, ee=R.EE[:6]), dict(kind=1, aux=None, ee=R.EE[6:12]), dict(kind=2, aux=None),
               dict(resident=2, null=("text", "idx"), idx=None, n_records=6, nsel=6, aux=None, ee=np.zeros(6)),
               dict(text=b"", idx=np.zeros((0, 6)), aux=np.zeros((0, 3)), null=("text",))):
        assert "ctx is NULL" in entry_call(**kw)[1], kw


def test_an_ee_outside_the_domain_is_said_with_its_position_before_the_context_is_looked_at():
    for kind, aux in ((0, None), (1, None), (2, None), (4, AUX)):
        for v in R.OUTSIDE:
            ee = np.array([0.5, 1.0, 2.0, v, 3.0, float("nan")])
            rc, msg, bad = entry_call(kind=kind, aux=aux, ee=ee)
            assert rc == L.E_INVALID and bad == 3 and "ee[3]" in msg and "ctx is NULL" not in msg, (kind, v, msg)
        # ... in the resident form too: ee always comes from the host
        rc, msg, bad = entry_call(kind=kind, aux=None, resident=2, null=("text", "idx"), idx=None, n_records=6, nsel=6,
                                  ee=np.array([0.0, 0.0, 0.0, 0.0, 0.0, float(2 ** 53)]))
        assert rc == L.E_INVALID and bad == 5 and "ee[5]" in msg
    # the ends of the domain are taken
    assert "ctx is NULL" in entry_call(ee=np.array([float(2 ** 53 - 1), -float(2 ** 53 - 1), 5e-324, -0.0, 1e-300, 0.0]))[1]


def test_a_bad_row_is_said_with_its_record_before_the_context_is_looked_at():
    for c, bad in R.refused_cases():
        if c["name"].startswith("ee_outside"):
            continue                                         # (said as an ee: above)
        kw = c["kw"]
        rc, msg, got = entry_call(text=c["text"], idx=c["idx"], sel=c["sel"], kind=kw["kind"], relabel=(kw.get("relabel") or "").encode() or None,
                                  relabel_index=kw.get("relabel_index"), ee=kw.get("ee"), aux=kw.get("aux"))
        assert rc == L.E_INVALID and "selected record %d fails a check" % bad in msg and got == bad, c["name"]
    c = R.report_ignores_sequence_columns()
    assert "ctx is NULL" in entry_call(text=c["text"], idx=c["idx"], aux=c["kw"]["aux"], ee=c["kw"]["ee"])[1]


def test_the_old_entry_still_refuses_kind_4_in_its_own_name():
    rc, msg, _ = entry_call(entry="mpb_format_text_host", kind=4)
    assert rc == L.E_INVALID and "mpb_format_text_host: kind 4 is none of fasta (0), qual (1), fastq (2)" in msg and "report" not in msg
    assert "ctx is NULL" in entry_call(entry="mpb_format_text_host", kind=2)[1]


def test_the_entry_is_declared_as_its_prototype_says():
    hdr = open(os.path.join(ROOT, "include", "moira_pb.h")).read()
    assert "#define MPB_K_COUNT     22" in hdr
    old = hdr[hdr.index("int mpb_format_text_host("):].split(";")[0]
    new = hdr[hdr.index("int mpb_format_records_host("):].split(";")[0]
    assert len(L.PROTOTYPES["mpb_format_records_host"][1]) == new.count(",") + 1 == old.count(",") + 3
    assert "const double *ee, const int32_t *aux, int32_t bgzf" in " ".join(new.split())
    strip = lambda d: " ".join(d.split()).replace("const double *ee, const int32_t *aux, ", "").replace("mpb_format_records_host", "mpb_format_text_host")
    assert strip(new) == strip(old)                          # all of the old entry's arguments, in its order
    doc = hdr[hdr.index("RESIDENT FORM"):hdr.index("int mpb_format_text_host(")]
    for word in ("THE CONTIG GENERATION", "*n_handed_back == 0", "mpb_contigs_text_host", "mpb_contigs_filter_text_host", "single-end generation"):
        assert word in doc, word
    src = open(os.path.join(ROOT, "moira_amd", "csrc", "mpb_contig.cpp")).read()
    assert src.count("resident_drop_contigs(c);") == 1 and src.count("resident_keep_contigs(c, ") == 1
    lane = open(os.path.join(ROOT, "moira_amd", "csrc", "mpb_format_lane.inc")).read()
    assert "#define FM_KIND_REPORT 4" in lane and F.FMT_REPORT == 4


# ---- the switches -----------------------------------------------------------------------------------------------------------------

def fake_backend(text=True, report=True, collapse=True):
    be = lambda *a, **k: None
    be.engine = types.SimpleNamespace(device=0, filter_fastq=None)
    if text:
        be.engine.format_text = lambda *a, **k: None
    if report:
        be.engine.format_report = lambda *a, **k: None
    if collapse:
        be.engine.collapse_text = lambda *a, **k: None
    return be


def test_eligibility_of_both_switches():
    from test_cli_golden import reference_args
    fq = os.path.join(GOLD, "test1.fastq.gz")
    single, paired_on = {"device_index", "device_pack"}, {"device_contigs", "device_pack", "device_pair_index"}
    s = lambda **kw: reference_args(paired=False, forward_fastq=fq, **kw)
    p = lambda **kw: reference_args(paired=True, forward_fastq=fq, reverse_fastq=fq, **kw)
    fmt, col = cli._device_format_eligible, cli._device_collapse_eligible
    # new: USEARCH single-end with the ee-capable engine; paired with --device_pair_index in force
    assert fmt(s(collapse=False, pipeline="USEARCH"), fake_backend(), single)
    assert not fmt(s(collapse=False, pipeline="USEARCH"), fake_backend(report=False), single)
    assert fmt(p(collapse=False), fake_backend(), paired_on) and fmt(p(collapse=False, pipeline="USEARCH"), fake_backend(), paired_on)
    assert not fmt(p(collapse=False), fake_backend(report=False), paired_on)
    assert not fmt(p(collapse=False), fake_backend(), {"device_contigs", "device_pack"})           # the host-indexed paired path
    assert not fmt(p(collapse=True), fake_backend(), paired_on)
    assert col(p(collapse=True), fake_backend(), paired_on)
    assert not col(p(collapse=True), fake_backend(), {"device_contigs", "device_pack"})
    assert not col(p(collapse=True), fake_backend(collapse=False), paired_on)
    assert not col(p(collapse=False), fake_backend(), paired_on)
    # pinned: the single-end cases as they were
    assert fmt(s(collapse=False), fake_backend(), single) and fmt(s(collapse=False), fake_backend(report=False), single)
    assert not fmt(s(collapse=False), fake_backend(), {"device_pack"}) and not fmt(s(collapse=False), fake_backend(text=False), single)
    assert not fmt(s(collapse=True), fake_backend(), single)
    assert col(s(collapse=True), fake_backend(), single) and not col(s(collapse=False), fake_backend(), single)
    assert not col(p(collapse=True), fake_backend(), single)                                       # (paired never goes on from --device_index)


def test_the_sentences_and_the_help_name_the_paired_form():
    for sentence, switch in ((cli.DEVICE_FORMAT_SENTENCE, "--device_format"), (cli.DEVICE_COLLAPSE_SENTENCE, "--device_collapse")):
        assert sentence.startswith(switch + " does not apply to this run (") and "paired with --device_pair_index" in sentence
        assert "single-end with --device_index and --device_pack" in sentence
    assert "-c false" in cli.DEVICE_FORMAT_SENTENCE and "-c true" in cli.DEVICE_COLLAPSE_SENTENCE
    assert "mothur" not in cli.DEVICE_FORMAT_SENTENCE
    text = " ".join(cli.build_parser().format_help().split())
    assert "paired with --device_pair_index" in text and "contigs.report" in text


# ---- the consumer's side, with an engine made of the host functions ----------------------------------------------------------------

class HostEngine:
    """contigs_filter_fastq = fastio.index x 2 + the host aligner + the backend's text filter, every pair done and filtered; the
    contigs of the last call are `resident` under a generation number (none for the calls listed in no_generation), and
    format_text / format_report / collapse_text are the host functions on them -- NotResident for any other generation."""
    device = 0
    contigs_text = contigs_filter_text = None

    def __init__(self, text_filter, no_generation=()):
        self.filter, self.none, self.calls, self.gen, self.last, self.kept, self.seen = text_filter, set(no_generation), 0, 0, 0, None, []

    def contigs_filter_fastq(self, fbuf, rbuf, ffinal, rfinal, max_records, fastq_offset, *aln, max_len=0, lower_n_is_base=False, **kw):
        k, self.calls = self.calls, self.calls + 1
        f, r = F.index(fbuf, ffinal, max_records), F.index(rbuf, rfinal, max_records)
        n = min(len(f[0]), len(r[0]))
        mis = F.first_header_mismatch(fbuf, f[0][:n], rbuf, r[0][:n]) if n else -1
        nb = n if mis < 0 else mis
        cons = [F.index(b, fin, n)[1] if n else 0 for b, fin in ((fbuf, ffinal), (rbuf, rfinal))]
        cbuf, cidx, aux = CT.contigs_from_fastq(fbuf, f[0][:nb], rbuf, r[0][:nb], fastq_offset, threads=2)
        ee, has_n = self.filter(cbuf, cidx, fastq_offset, max_len, lower_n_is_base) if nb else (np.zeros(0), np.zeros(0, bool))
        self.gen = 0
        if nb and k not in self.none:
            self.last += 1
            self.gen, self.kept = self.last, (bytes(cbuf), cidx.copy(), aux.copy())
        return types.SimpleNamespace(
            fidx=f[0], ridx=r[0], f_bad=f[2], r_bad=r[2], f_consumed=cons[0], r_consumed=cons[1], mismatch=mis, n_pairs=n, n_built=nb,
            rec_cap=len(cbuf) // max(nb, 1), cbuf=cbuf, cidx=cidx, aux=aux, done=np.ones(nb, bool), ee=ee, has_n=has_n,
            filtered=np.ones(nb, bool), filter_error=None, resident=self.gen)

    def _held(self, resident):
        if not resident or resident != self.gen:
            raise E.NotResident("text %d is not resident" % resident)
        return self.kept

    def format_text(self, buf=None, idx=None, sel=None, kind=2, resident=None, bgzf=False, **kw):
        cbuf, cidx, _ = self._held(resident)
        assert buf is None and not bgzf and np.array_equal(idx, cidx)
        self.seen.append(("text", kind, resident, len(cidx) if sel is None else len(sel)))
        return bytes(F.format_records(cbuf, cidx, np.arange(len(cidx)) if sel is None else sel, kind, **kw))

    def format_report(self, buf=None, idx=None, aux=None, sel=None, resident=None, bgzf=False, **kw):
        cbuf, cidx, kept_aux = self._held(resident)
        assert buf is None and aux is None and sel is None and not bgzf and np.array_equal(idx, cidx)
        self.seen.append(("report", F.FMT_REPORT, resident, len(cidx)))
        return bytes(F.format_report(cbuf, cidx, np.arange(len(cidx)), kept_aux, **kw))


def host_backend(oracle, **kw):
    from test_cli_golden import oracle_backend
    be = oracle_backend(oracle)

    def text(buf, idx, alpha, ambigs, round_, in_off, T, n_is_base, method=None, fast_discard=None, sel=None):
        sel = np.arange(len(idx)) if sel is None else np.asarray(sel)
        lens = np.minimum(idx[sel, F.SEQ_LEN], T) if T else idx[sel, F.SEQ_LEN]
        q, ln, fl = F.pack_parallel(None, 1, buf, idx, sel, in_off, T, n_is_base, 64 * ((int(lens.max()) + 63) // 64))
        return be.matrix(q, ln, alpha, ambigs, round_), fl
    be.text = text
    be.text_choice = lambda *a, **k: {}
    be.engine = HostEngine(lambda cbuf, cidx, off, T, n_is_base: text(cbuf, cidx, 0.005, "treat_as_errors", False, off, T, n_is_base), **kw)
    return be


OUTPUTS = ("qc.good.fasta", "qc.good.qual", "qc.bad.fasta", "qc.bad.qual", "contigs.report")


def paired_run(tmp_path, oracle, name, pipeline="mothur", **kw):
    from test_cli_golden import reference_args
    log = io.StringIO()
    be = host_backend(oracle, **{k: kw.pop(k) for k in ("no_generation",) if k in kw})
    a = reference_args(paired=True, forward_fastq=os.path.join(GOLD, "test1.fastq.gz"), reverse_fastq=os.path.join(GOLD, "test2.fastq.bz2"),
                       output_prefix=str(tmp_path / name), collapse=False, pipeline=pipeline, silent=False, device_contigs=True,
                       device_pack=True, device_pair_index=True, **kw)
    assert cli.main(a, backend=be, out=log) == 0
    files = {k: open("%s.%s" % (tmp_path / name, k), "rb").read() for k in OUTPUTS}
    assert files["contigs.report"].count(b"\n") == 1001 and files["qc.good.fasta"]
    return files, be.engine, log.getvalue()


@pytest.mark.parametrize("pipeline", ["mothur", "USEARCH"])
def test_a_paired_chunk_with_a_generation_is_formatted_through_the_engine_report_included(tmp_path, oracle, monkeypatch, pipeline):
    monkeypatch.setattr(cli, "PAIR_CHUNK_READS", 300)        # four chunks
    want, eng0, log0 = paired_run(tmp_path, oracle, "host", pipeline)
    assert eng0.calls >= 4 and eng0.seen == [] and "does not apply" not in log0
    got, eng, log = paired_run(tmp_path, oracle, "device", pipeline, device_format=True)
    assert got == want
    assert "does not apply" not in log and "--device_format:" not in log
    if pipeline == "USEARCH":
        assert b";ee=" in got["contigs.report"] and b";size=1;" in got["qc.good.fasta"]
    # every chunk: its report lines, and fasta + qual of the kept and of the discarded records, all on the chunk's own generation
    chunks = sorted({s[2] for s in eng.seen})
    assert chunks == list(range(1, eng.last + 1)) and eng.last >= 4      # one generation per contig call that yielded a chunk
    for g in chunks:
        mine = [s for s in eng.seen if s[2] == g]
        assert mine[0][0] == "report" and sum(1 for s in mine if s[0] == "report") == 1
        kinds = sorted(s[1] for s in mine[1:])
        assert kinds in ([F.FMT_FASTA, F.FMT_QUAL], [F.FMT_FASTA, F.FMT_FASTA, F.FMT_QUAL, F.FMT_QUAL])
    assert sum(s[3] for s in eng.seen if s[0] == "report") == 1000


def test_a_chunk_without_a_generation_goes_the_host_way_said_once(tmp_path, oracle, monkeypatch):
    monkeypatch.setattr(cli, "PAIR_CHUNK_READS", 300)
    want, _, _ = paired_run(tmp_path, oracle, "host")
    got, eng, log = paired_run(tmp_path, oracle, "device", device_format=True, no_generation={1, 2})
    assert got == want
    said = [l for l in log.splitlines() if l.startswith("--device_format: a chunk was not formatted on the device")]
    assert len(said) == 1 and "it came the host way" in said[0]
    assert len({s[2] for s in eng.seen}) == eng.calls - 2 >= 2 and 0 not in {s[2] for s in eng.seen}
