"""What of the device collapse step needs no device: the argument checks of mpb_collapse_text_host (made before the context is
looked at) and its host-side row validation, the prototype against the header's declaration, the build lists, and the CLI's
--device_collapse switch and its eligibility.  The lane code on the host: tests/test_collapse_lane_model.py; the grouped host
entry: tests/test_collapse_grouped.py; the kernels: tests/test_gpu_collapse_text.py."""
import ctypes as C
import io
import os
import types

import numpy as np

from helpers import collapse_inputs as X
from moira_amd import _lib as L
from moira_amd import build as B
from moira_amd import cli

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
TEXT, IDX = X.raw([b"ACGT", b"ACGT", b"TT"])


def entry_call(null=(), text=TEXT, idx=IDX, text_bytes=None, n_records=None, resident=0, max_len=0):
    lib = L.load()
    idx = None if idx is None else np.ascontiguousarray(idx, np.int64)
    n = (0 if idx is None else len(idx)) if n_records is None else n_records
    h, rep, bad = np.full(8, 7, np.uint64), np.full(8, 7, np.int32), C.c_int64(-7)
    rc = lib.mpb_collapse_text_host(None, None if "text" in null else text, len(text or b"") if text_bytes is None else text_bytes,
                                    None if "idx" in null or idx is None else idx.ctypes.data, n, resident, max_len,
                                    None if "hash" in null else h.ctypes.data, None if "rep" in null else rep.ctypes.data,
                                    None if "bad_record" in null else C.byref(bad))
    assert (h == 7).all() and (rep == 7).all()               # nothing is written without a context
    return rc, lib.mpb_last_error().decode(), bad.value


def test_argument_errors_are_invalid_with_or_without_a_device():
    rc, msg, bad = entry_call()
    assert rc == L.E_INVALID and "ctx is NULL" in msg and bad == -1          # good arguments: only the context is missing
    cases = [(dict(null=("idx",)), "either text and idx"), (dict(null=("text",)), "either text and idx"),
             (dict(null=("hash",)), "bad arguments"), (dict(null=("rep",)), "bad arguments"), (dict(null=("bad_record",)), "bad arguments"),
             (dict(text_bytes=-1), "bad arguments"), (dict(n_records=-1), "bad arguments"), (dict(max_len=-1), "max_len -1 is negative"),
             (dict(resident=3), "not both or neither"), (dict(resident=-1, null=("text", "idx")), "is no generation"),
             (dict(resident=3, null=("text",)), "not both or neither"), (dict(resident=3, null=("idx",)), "not both or neither"),
             (dict(resident=2, null=("text", "idx"), n_records=1 << 31), "at most 2147483647"),
             (dict(text_bytes=(1 << 30) + 1), "at most 1073741824 bytes (1 GiB)")]
    for kw, what in cases:
        rc, msg, _ = entry_call(**kw)
        assert rc == L.E_INVALID and "ctx is NULL" not in msg and what in msg, (kw, msg)
    # what is taken: the resident form, no records at all (with and without the arrays), an empty text
    for kw in (dict(resident=9, null=("text", "idx"), idx=None, n_records=3), dict(idx=np.zeros((0, 6)), null=("hash", "rep")),
               dict(idx=np.zeros((0, 6))), dict(text=b"", idx=np.zeros((0, 6)), null=("text",)), dict(max_len=1 << 30)):
        assert "ctx is NULL" in entry_call(**kw)[1], kw


def test_a_bad_row_is_said_with_its_record_before_the_context_is_looked_at():
    for c, bad in X.bad_row_cases():
        rc, msg, got = entry_call(text=c["text"], idx=c["idx"])
        assert rc == L.E_INVALID and "record %d fails a check" % bad in msg and got == bad, c["name"]
    # the other four columns are not the step's business
    idx = IDX.copy()
    idx[:, [0, 1, 4, 5]] = -5
    assert "ctx is NULL" in entry_call(idx=idx)[1]


def test_the_entry_is_declared_as_its_prototype_says_and_the_unit_is_built():
    hdr = open(os.path.join(ROOT, "include", "moira_pb.h")).read()
    decl = hdr[hdr.index("int mpb_collapse_text_host("):].split(";")[0]
    proto = L.PROTOTYPES["mpb_collapse_text_host"]
    assert proto[0] is C.c_int and len(proto[1]) == decl.count(",") + 1 == 10
    by_width = {"int64_t": C.c_int64, "int32_t": C.c_int32}
    for arg, ctype in zip(decl[decl.index("(") + 1:].rstrip(")").split(","), proto[1]):
        if "*" not in arg:
            assert ctype is by_width[arg.split()[0]], arg
        else:
            assert ctype in (C.c_void_p, C.POINTER(C.c_int64)), arg
    io_hdr = open(os.path.join(ROOT, "include", "moira_io.h")).read()
    decl = io_hdr[io_hdr.index("int32_t mio_collapse_add_grouped("):].split(";")[0]
    from moira_amd import fastio as F
    assert len(F.PROTOTYPES["mio_collapse_add_grouped"][1]) == decl.count(",") + 1 == 11
    assert "result is correct iff hash[] is right and rep[k] != k implies equal bytes" in io_hdr
    names = [os.path.basename(p) for p in B.SOURCES]
    assert "mpb_collapse_kernels.hip" in names and "mpb_collapse.cpp" in names
    assert "mpb_collapse_lane.inc" in [os.path.basename(p) for p in B.DEPS]
    assert "#define MPB_K_COUNT     22" in hdr               # no timing id of its own: the kernels' header says where they are timed
    unit = open(os.path.join(ROOT, "moira_amd", "csrc", "mpb_collapse_kernels.hip")).read()
    assert "MPB_K_PACK_TEXT" in unit and "return values of its two atomics" in unit


# ---- the switch ------------------------------------------------------------------------------------------------------------------

def test_the_parser_knows_the_switch_and_it_goes_through_the_paths_owner():
    p = cli.build_parser()
    off, on = p.parse_args(["-ffq", "a"]), p.parse_args(["-ffq", "a", "--device_collapse"])
    assert off.device_collapse is False and on.device_collapse is True and "--device_collapse" in p.format_help()
    assert cli._DevicePaths().collapse is False and cli._DevicePaths(("device_pack", "device_index")).collapse is False
    said = []
    d = cli._DevicePaths({"device_pack", "device_index", "device_collapse"}, 0, said.append)
    assert d.collapse and d.engine is None and not d.format
    d.collapse_refused("it came the host way"), d.collapse_refused("again")
    assert said == ["--device_collapse: a chunk was not hashed and grouped on the device (it came the host way): the host collapse "
                    "does both for it."]


def fake_backend(call=True):
    be = lambda *a, **k: None
    be.engine = types.SimpleNamespace(device=0, filter_fastq=None)
    if call:
        be.engine.collapse_text = lambda *a, **k: None
    return be


def test_eligibility():
    from test_cli_golden import reference_args
    fq = os.path.join(GOLD, "test1.fastq.gz")
    both = {"device_index", "device_pack"}
    a = reference_args(paired=False, forward_fastq=fq, collapse=True)
    assert cli._device_collapse_eligible(a, fake_backend(), both)
    assert cli._device_collapse_eligible(reference_args(paired=False, forward_fastq=fq, collapse=True, truncate=100, pipeline="USEARCH"),
                                         fake_backend(), both)
    assert not cli._device_collapse_eligible(a, fake_backend(), {"device_pack"})
    assert not cli._device_collapse_eligible(a, fake_backend(), {"device_index"})
    assert not cli._device_collapse_eligible(a, fake_backend(call=False), both)
    assert not cli._device_collapse_eligible(reference_args(paired=False, forward_fastq=fq, collapse=False), fake_backend(), both)
    assert not cli._device_collapse_eligible(reference_args(paired=True, forward_fastq=fq, reverse_fastq=fq, collapse=True), fake_backend(), both)


def test_the_switch_says_its_sentence_where_it_does_not_apply_and_the_output_is_unchanged(tmp_path, oracle):
    from test_cli_golden import oracle_backend, reference_args, same_files
    for name, kw, want in (("off", {}, []), ("on", dict(device_collapse=True), ["--device_collapse"]),
                           ("all", dict(device_collapse=True, device_index=True, device_pack=True),
                            ["--device_pack", "--device_index", "--device_collapse"]),
                           ("quiet", dict(device_collapse=True, nowarnings=True), [])):
        log = io.StringIO()
        a = reference_args(paired=False, forward_fastq=os.path.join(GOLD, "test1.fastq.gz"), output_prefix=str(tmp_path / name), **kw)
        assert cli.main(a, backend=oracle_backend(oracle), out=log) == 0
        lines = [l for l in log.getvalue().splitlines() if "does not apply to this run" in l]
        assert [l.split(" ")[0] for l in lines] == want
        if want:
            assert lines[-1] == cli.DEVICE_COLLAPSE_SENTENCE
        same_files(str(tmp_path / name), "forward")
