"""The CLI with --device_collapse on the GPU: the golden single-end run with --device_pack --device_index, collapsing (-c true,
the default), at -p 1 and -p 16, with and without -t 100.  Every output file must be byte-equal to the run without the switch,
and the run with the reference's own flags byte-equal to tests/golden/reference_test_results/forward.*.  The matrix runs in this
process on one backend (a process of its own per run would pay the context's start-up nine times); one run goes through
moira.py as a command, under its own timeout.  A chunk that comes the host way, or whose call finds its generation stale, takes
the host collapse and says so once.  A run where the switch does not apply (-c false) says its sentence and writes what it
wrote.  The entry itself: tests/test_gpu_collapse_text.py."""
import io
import os
import subprocess
import sys

import pytest

from moira_amd import cli
from moira_amd import engine as E

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
SRC = os.path.join(GOLD, "test1.fastq.gz")
KINDS = ("good.fasta", "good.qual", "good.names", "bad.fasta", "bad.qual", "bad.names")


@pytest.fixture(scope="module")
def backend():
    be = cli.make_gpu_backend(None)
    yield be
    be.engine.close()


def files_of(tmp_path, name):
    out = {}
    for p in sorted(os.listdir(str(tmp_path))):
        if p.startswith(name + "."):
            out[p.split(".", 1)[1]] = open(os.path.join(str(tmp_path), p), "rb").read()
    return out


def run_cli(backend, tmp_path, name, on, processors=4, hand_back=None, stale=None, **kw):
    """-> (the files; the log; the records of the collapse calls the engine saw).  hand_back: the filter_fastq call (counted from
    0) that raises NotTaken with a reason the host indexer has no quarrel with, so that block comes the host way; stale: the
    collapse_text call that raises NotResident."""
    from test_cli_golden import reference_args
    kw.setdefault("collapse", True)
    a = reference_args(paired=False, forward_fastq=SRC, output_prefix=str(tmp_path / name), processors=processors, device_pack=True,
                       device_index=True, device_collapse=on, **kw)
    seen, calls = [], dict(filter=0, collapse=0)
    inner, inner_filter = backend.engine.collapse_text, backend.engine.filter_fastq

    def collapse_text(*x, **k):
        calls["collapse"] += 1
        if stale is not None and calls["collapse"] - 1 == stale:
            raise E.NotResident("made stale by the test")
        r = inner(*x, **k)
        seen.append((len(r[1]), k.get("max_len")))
        return r

    def filter_fastq(*x, **k):
        calls["filter"] += 1
        if hand_back is not None and calls["filter"] - 1 == hand_back:
            raise E.NotTaken(4)
        return inner_filter(*x, **k)
    backend.engine.collapse_text, backend.engine.filter_fastq = collapse_text, filter_fastq
    log = io.StringIO()
    try:
        assert cli.main(a, backend=backend, out=log) == 0
    finally:
        backend.engine.collapse_text, backend.engine.filter_fastq = inner, inner_filter
    return files_of(tmp_path, name), log.getvalue(), seen


def golden_files():
    res = os.path.join(GOLD, "reference_test_results")
    return {"qc." + k: open(os.path.join(res, "forward.qc." + k), "rb").read() for k in KINDS}


OFF = {}


@pytest.mark.parametrize("truncate", [None, 100])
@pytest.mark.parametrize("processors", [1, 16])
def test_output_files_are_identical_with_and_without_the_switch(backend, tmp_path, processors, truncate):
    if truncate not in OFF:                                  # (the run without the switch: once per option)
        OFF[truncate] = run_cli(backend, tmp_path, "off", False, truncate=truncate)
        assert OFF[truncate][2] == []
    off = OFF[truncate][0]
    on, log, seen = run_cli(backend, tmp_path, "on", True, processors=processors, truncate=truncate)
    assert off.keys() == on.keys() and len(on) == 6 and off == on
    assert "--device_collapse" not in log, log
    assert seen == [(1000, truncate or 0)]                   # every record's hash and rep came from the device
    if truncate is None:
        assert on == golden_files()                          # the reference's own flags: the reference's own files


def test_a_chunk_that_comes_the_host_way_takes_the_host_collapse_between_device_chunks(backend, tmp_path, monkeypatch):
    monkeypatch.setattr(cli, "DEVICE_INDEX_BLOCK", 100000)
    off, _, _ = run_cli(backend, tmp_path, "off", False)
    on, log, seen = run_cli(backend, tmp_path, "on", True, processors=16, hand_back=2)
    assert off == on == golden_files()
    assert log.count("--device_index: the device did not take a block (row check)") == 1
    assert log.count("--device_collapse") == 1, log
    assert log.count("--device_collapse: a chunk was not hashed and grouped on the device (it came the host way): the host collapse "
                     "does both for it.") == 1
    assert len(seen) >= 3 and 500 < sum(n for n, _ in seen) < 1000       # device chunks on both sides of it


def test_a_call_that_finds_its_generation_stale_takes_the_host_collapse_for_that_chunk(backend, tmp_path, monkeypatch):
    monkeypatch.setattr(cli, "DEVICE_INDEX_BLOCK", 100000)
    on, log, seen = run_cli(backend, tmp_path, "on", True, stale=1)
    assert on == golden_files()
    assert log.count("--device_collapse") == 1 and log.count("a chunk was not hashed and grouped on the device (made stale by the test)") == 1, log
    assert len(seen) >= 3 and 0 < sum(n for n, _ in seen) < 1000


def test_without_collapse_the_switch_says_its_sentence_and_the_output_is_unchanged(backend, tmp_path):
    off, _, _ = run_cli(backend, tmp_path, "off", False, collapse=False)
    on, log, seen = run_cli(backend, tmp_path, "on", True, collapse=False)
    assert off == on and len(on) >= 4 and seen == []
    assert log.count("--device_collapse") == 1 and log.count(cli.DEVICE_COLLAPSE_SENTENCE) == 1, log


def test_the_command_line_takes_the_switch(tmp_path):
    cmd = [sys.executable, os.path.join(ROOT, "moira.py"), "-ffq", SRC, "--silent", "-p", "16", "-op", str(tmp_path / "cmd"),
           "--device_pack", "--device_index", "--device_collapse"]
    p = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert p.returncode == 0 and "--device_collapse" not in p.stdout + p.stderr, p.stdout[-2000:] + p.stderr[-2000:]
    assert files_of(tmp_path, "cmd") == golden_files()
