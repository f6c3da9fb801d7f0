"""What of the device formatter needs no device: the argument checks of mpb_format_text_host (made before the context is looked
at) and its host-side row validation, the pinned kernel count and path table, the CLI's --device_format switch and its
eligibility, and _BlockCompressedWriter.write_members.  The lane code on the host: tests/test_format_lane_model.py; the
kernels: tests/test_gpu_format_text.py."""
import ctypes as C
import gzip
import io
import os
import types

import numpy as np

from helpers import format_inputs as X
from moira_amd import _lib as L
from moira_amd import cli
from moira_amd import fastio as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
TEXT, IDX = X.count_text(6, 3)


def entry_call(null=(), text=TEXT, idx=IDX, text_bytes=None, n_records=None, resident=0, sel=None, nsel=None, kind=2, offset=33,
               out_offset=33, max_len=0, relabel=None, relabel_index=None, labels=None, n_labels=None, label_id=None, bgzf=0,
               out_cap=1 << 16):
    lib = L.load()
    out = np.zeros(1 << 16, np.uint8)
    got, needed, bad = C.c_int64(-7), C.c_int64(-7), C.c_int64(-7)
    idx = None if idx is None else np.ascontiguousarray(idx, np.int64)
    keep = [np.ascontiguousarray(a, t) if a is not None else None for a, t in ((sel, np.int64), (relabel_index, np.int64), (label_id, np.int32))]
    ptr = lambda a: None if a is None else a.ctypes.data
    enc = [s.encode() for s in labels or []]
    lab = (C.c_char_p * max(len(enc), 1))(*enc)
    rc = lib.mpb_format_text_host(
        None, None if "text" in null else text, len(text or b"") if text_bytes is None else text_bytes, None if "idx" in null else ptr(idx),
        (0 if idx is None else len(idx)) if n_records is None else n_records, resident, ptr(keep[0]),
        (len(sel) if sel is not None else 0 if idx is None else len(idx)) if nsel is None else nsel, kind, offset, out_offset, 1, max_len,
        relabel, ptr(keep[1]), C.cast(lab, C.c_void_p) if labels is not None else None, len(enc) if n_labels is None else n_labels,
        ptr(keep[2]), bgzf, None if "out" in null else out.ctypes.data, out_cap, None if "out_bytes" in null else C.byref(got),
        None if "text_needed" in null else C.byref(needed), None if "bad_record" in null else C.byref(bad), None)
    return rc, lib.mpb_last_error().decode(), bad.value


def test_argument_errors_are_invalid_with_or_without_a_device():
    rc, msg, bad = entry_call()
    assert rc == L.E_INVALID and "ctx is NULL" in msg and bad == -1          # good arguments: only the context is missing
    cases = [(dict(null=("idx",)), "either text and idx"), (dict(null=("text",)), "either text and idx"),
             (dict(null=("out",)), "bad arguments"), (dict(null=("out_bytes",)), "bad arguments"),
             (dict(null=("text_needed",)), "bad arguments"), (dict(null=("bad_record",)), "bad arguments"),
             (dict(text_bytes=-1), "bad arguments"), (dict(n_records=-1), "bad arguments"), (dict(nsel=-1), "bad arguments"),
             (dict(out_cap=-1), "bad arguments"), (dict(kind=-1), "kind -1"), (dict(kind=3), "kind 3"),
             (dict(offset=-1), "outside 0..255"), (dict(offset=256), "outside 0..255"), (dict(out_offset=-1), "outside 0..255"),
             (dict(out_offset=256), "outside 0..255"), (dict(relabel=b"S"), "relabel without relabel_index"),
             (dict(label_id=np.zeros(6)), "label_id without labels"), (dict(label_id=np.zeros(6), labels=[]), "label_id without labels"),
             (dict(labels=["a"] * 17, label_id=np.zeros(6)), "17 labels: at most 16"), (dict(labels=["a"], n_labels=-1), "labels: at most 16"),
             (dict(labels=["a", "b" * 256], label_id=np.zeros(6)), "a label is longer than 255 bytes"),
             (dict(relabel=b"R" * 256, relabel_index=np.arange(6)), "relabel is longer than 255 bytes"),
             (dict(max_len=-1), "max_len -1 is negative"),
             (dict(resident=3), "not both or neither"), (dict(resident=-1, null=("text", "idx")), "is no generation"),
             (dict(text_bytes=(1 << 30) + 1), "at most 1073741824 bytes (1 GiB)")]
    for kw, what in cases:
        rc, msg, _ = entry_call(**kw)
        assert rc == L.E_INVALID and "ctx is NULL" not in msg and what in msg, (kw, msg)
    # the limits themselves are taken: 16 labels of 255 bytes, a relabel of 255 bytes, every offset
    for kw in (dict(labels=["b" * 255] * 16, label_id=np.arange(6)), dict(relabel=b"R" * 255, relabel_index=np.arange(6)),
               dict(offset=0, out_offset=255), dict(resident=9, null=("text", "idx"), idx=None, n_records=4, nsel=0),
               dict(text=b"", idx=np.zeros((0, 6)), null=("text",))):
        assert "ctx is NULL" in entry_call(**kw)[1], kw


def test_a_bad_row_is_said_with_its_record_before_the_context_is_looked_at():
    for c, bad in X.damaged_cases():
        kw = c["kw"]
        rc, msg, got = entry_call(text=c["text"], idx=c["idx"], sel=c["sel"], kind=kw["kind"], relabel=(kw.get("relabel") or "").encode() or None,
                                  relabel_index=kw.get("relabel_index"), labels=kw.get("labels"), label_id=kw.get("label_id"))
        assert rc == L.E_INVALID and "selected record %d fails a check" % bad in msg and got == bad, c["name"]
    c = X.fasta_ignores_quality_columns()
    assert "ctx is NULL" in entry_call(text=c["text"], idx=c["idx"], kind=F.FMT_FASTA)[1]


def test_the_entry_is_declared_and_the_pinned_tables_keep_their_length():
    hdr = open(os.path.join(ROOT, "include", "moira_pb.h")).read()
    assert "#define MPB_K_COUNT     22" in hdr
    decl = hdr[hdr.index("int mpb_format_text_host("):].split(";")[0]
    assert len(L.PROTOTYPES["mpb_format_text_host"][1]) == decl.count(",") + 1
    assert "int64_t mpb_resident_text(mpb_ctx *ctx);" in hdr and L.PROTOTYPES["mpb_resident_text"][0] is C.c_int64
    kernels = list(L.KERNEL_NAMES) + list(L.CONTIG_KERNEL_NAMES) + list(L.BGZF_KERNEL_NAMES) + list(L.INFLATE_KERNEL_NAMES) + list(L.INDEX_KERNEL_NAMES)
    assert sorted(kernels) == list(range(22)) and len(L.FQ_WHY) == 5 and len(L.BGZF_WHY) == 14
    # every call the header lists as dropping the resident text does so in the library's source
    doc = hdr[hdr.index("RESIDENT FORM"):hdr.index("int mpb_format_text_host(")]
    for entry, unit in (("mpb_fastq_index_host", "mpb_index.cpp"), ("mpb_filter_fastq_host", "mpb_index.cpp"),
                        ("mpb_filter_bgzf_fastq_host", "mpb_bgzf_fastq.cpp"), ("mpb_contigs_filter_fastq_host", "mpb_contig.cpp")):
        src = open(os.path.join(ROOT, "moira_amd", "csrc", unit)).read()
        body = src[src.index("int %s(" % entry):]
        assert entry in doc and "resident_drop(c);" in body[:body.index("StreamQueue q(c)")], entry


# ---- the switch ------------------------------------------------------------------------------------------------------------------

def test_the_parser_knows_the_switch_and_the_table_keeps_its_five_rows():
    p = cli.build_parser()
    off, on = p.parse_args(["-ffq", "a"]), p.parse_args(["-ffq", "a", "--device_format"])
    assert off.device_format is False and on.device_format is True and "--device_format" in p.format_help()
    assert [r[0] for r in cli._DEVICE_PATHS] == ["device_pack", "device_contigs", "device_index", "device_compress", "device_inflate"]
    assert cli._DevicePaths().format is False and cli._DevicePaths(("device_pack", "device_index")).format is False
    said = []
    d = cli._DevicePaths({"device_pack", "device_index", "device_format"}, 0, said.append)
    assert d.format and d.engine is None
    d.format_refused("it came the host way"), d.format_refused("again")
    assert said == ["--device_format: a chunk was not formatted on the device (it came the host way): the host formatter is used for it."]


def fake_backend(call=True):
    be = lambda *a, **k: None
    be.engine = types.SimpleNamespace(device=0, filter_fastq=None)
    if call:
        be.engine.format_text = lambda *a, **k: None
    return be


def test_eligibility():
    from test_cli_golden import reference_args
    fq = os.path.join(GOLD, "test1.fastq.gz")
    both = {"device_index", "device_pack"}
    a = reference_args(paired=False, forward_fastq=fq, collapse=False)
    assert cli._device_format_eligible(a, fake_backend(), both)
    assert not cli._device_format_eligible(a, fake_backend(), {"device_pack"})
    assert not cli._device_format_eligible(a, fake_backend(), {"device_index"})
    assert not cli._device_format_eligible(a, fake_backend(call=False), both)
    assert not cli._device_format_eligible(reference_args(paired=False, forward_fastq=fq, collapse=True), fake_backend(), both)
    assert not cli._device_format_eligible(reference_args(paired=False, forward_fastq=fq, collapse=False, pipeline="USEARCH"), fake_backend(), both)


def test_the_switch_resolves_after_the_table_and_says_its_sentence_where_it_does_not_apply(tmp_path, oracle):
    from test_cli_golden import oracle_backend, reference_args, same_files
    for name, kw, want in (("off", {}, []), ("on", dict(device_format=True), ["--device_format"]),
                           ("all", dict(device_format=True, device_index=True, device_pack=True),
                            ["--device_pack", "--device_index", "--device_format"]),
                           ("quiet", dict(device_format=True, nowarnings=True), [])):
        log = io.StringIO()
        a = reference_args(paired=False, forward_fastq=os.path.join(GOLD, "test1.fastq.gz"), output_prefix=str(tmp_path / name), **kw)
        assert cli.main(a, backend=oracle_backend(oracle), out=log) == 0
        lines = [l for l in log.getvalue().splitlines() if "does not apply to this run" in l]
        assert [l.split(" ")[0] for l in lines] == want
        if want:
            assert lines[-1] == cli.DEVICE_FORMAT_SENTENCE
        same_files(str(tmp_path / name), "forward")


# ---- the writer ------------------------------------------------------------------------------------------------------------------

def test_write_members_keeps_order_with_buffered_text_before_the_members(tmp_path):
    rng = np.random.default_rng(2)
    parts = [bytes(rng.integers(65, 91, n, dtype=np.uint8).tolist()) for n in (10, (1 << 20) + 5, 70000, 3, 0, 200000)]
    for compressor in (None, types.SimpleNamespace(compress=lambda data: cli.bgzf_compress(data, 1))):
        path = str(tmp_path / ("m%d.gz" % (compressor is not None)))
        w = cli._BlockCompressedWriter(path, "gz", compressor)
        want = b""
        for i, part in enumerate(parts):
            if i % 2 == 0:
                w.write(part)                                # (text: buffered up to a block, or a batch)
            else:
                assert w.write_members(cli.bgzf_compress(part, 4)) >= 0      # whole members made elsewhere
            want += part
        w.write(b"tail")
        w.close()
        assert gzip.open(path, "rb").read() == want + b"tail"
        assert open(path, "rb").read().endswith(cli.BGZF_EOF)
    b = cli._BlockCompressedWriter(str(tmp_path / "x.bz2"), "bz2")
    try:
        b.write_members(b"")
        assert False, "a .bz2 output takes no members"
    except ValueError:
        pass
    b.close()
