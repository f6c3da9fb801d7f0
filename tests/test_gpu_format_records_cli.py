"""The CLI with --device_format and --device_collapse on paired input, and --device_format with the USEARCH pipeline, on the GPU:
output files must be identical (.gz: after decompression) with and without the switch.  The golden pairs run in chunks of 300
with --device_contigs --device_pack --device_pair_index, so every chunk's contigs stay on the device as a generation; a spy sees
the fasta / qual / fastq and report calls, and the grouped add of the collapse.  A pair with a 385-base mate is handed back:
its chunk goes the host way, said once.  The entry itself: tests/test_gpu_format_records.py."""
import gzip
import io
import os

import pytest

from helpers import pair_index_inputs as PI
from moira_amd import cli
from moira_amd import fastio as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def backend():
    be = cli.make_gpu_backend(None)
    yield be
    be.engine.close()


@pytest.fixture(scope="module")
def sources(tmp_path_factory):
    d = tmp_path_factory.mktemp("format_records_cli_src")
    f, r = PI.golden_texts()
    lines = f.split(b"\n")
    lines[4 * 450 + 1] = b"ACGT" * 96 + b"A"                 # pair 450 (the second chunk): 385 bases, more than the device takes
    lines[4 * 450 + 3] = b"I" * 385
    out = {}
    for name, text in (("forward", f), ("reverse", r), ("forward_385", b"\n".join(lines))):
        out[name] = str(d / (name + ".fastq"))
        with open(out[name], "wb") as fh:
            fh.write(text)
    return out


def run_cli(backend, tmp_path, name, forward, reverse=None, **kw):
    """-> (the files, decompressed where they are .gz; the log; what the engine's format and collapse calls saw)."""
    from test_cli_golden import reference_args
    gz = kw.get("output_compression") == "gz"
    paired = reverse is not None
    more = dict(device_contigs=True, device_pair_index=True) if paired else dict(device_index=True)
    a = reference_args(paired=paired, forward_fastq=forward, reverse_fastq=reverse, output_prefix=str(tmp_path / name), processors=4,
                       device_pack=True, device_compress=gz, silent=False, **dict(more, **kw))
    eng = backend.engine
    seen = []
    inner = dict(format_text=eng.format_text, format_report=eng.format_report, collapse_text=eng.collapse_text)

    def spy(what):
        def call(*x, **k):
            r = inner[what](*x, **k)
            seen.append((what, k.get("kind"), k.get("resident"), bool(k.get("bgzf")), k.get("ee") is not None))
            return r
        return call
    for what in inner:
        setattr(eng, what, spy(what))
    log = io.StringIO()
    try:
        assert cli.main(a, backend=backend, out=log) == 0
    finally:
        for what, fn in inner.items():
            setattr(eng, what, fn)
    files = {}
    for p in sorted(os.listdir(str(tmp_path))):
        if p.startswith(name + "."):
            path = os.path.join(str(tmp_path), p)
            files[p.split(".", 1)[1]] = gzip.open(path, "rb").read() if p.endswith(".gz") else open(path, "rb").read()
    return files, log.getvalue(), seen


PAIRED = [dict(), dict(output_format="fastq"), dict(output_compression="gz"), dict(pipeline="USEARCH", truncate=200, relabel="Seq")]


@pytest.mark.parametrize("kw", PAIRED, ids=["fasta", "fastq", "gz", "usearch"])
def test_paired_output_files_are_identical_with_and_without_device_format(backend, sources, tmp_path, monkeypatch, kw):
    monkeypatch.setattr(cli, "PAIR_CHUNK_READS", 300)        # four chunks
    off, log0, seen0 = run_cli(backend, tmp_path, "off", sources["forward"], sources["reverse"], collapse=False, **kw)
    on, log, seen = run_cli(backend, tmp_path, "on", sources["forward"], sources["reverse"], collapse=False, device_format=True, **kw)
    assert seen0 == [] and "does not apply" not in log0 + log and "--device_format" not in log, log
    assert off.keys() == on.keys() and len(on) >= 3 and off == on
    report = [v for k, v in on.items() if k.startswith("contigs.report")][0]
    assert report.count(b"\n") == 1001
    gz, usearch = kw.get("output_compression") == "gz", kw.get("pipeline") == "USEARCH"
    reports = [s for s in seen if s[0] == "format_report"]
    texts = [s for s in seen if s[0] == "format_text"]
    assert len(reports) == 4 and len({s[2] for s in reports}) == 4 and all(s[2] > 0 for s in seen)
    want_kinds = {F.FMT_FASTQ} if kw.get("output_format") == "fastq" else {F.FMT_FASTA, F.FMT_QUAL}
    assert {s[1] for s in texts} == want_kinds and len(texts) >= 4 * len(want_kinds)
    assert all(s[3] == gz and s[4] == usearch for s in seen)
    if usearch:
        assert b";ee=" in report and b";size=1;" in report


def test_paired_collapse_takes_the_grouped_add_on_the_contig_generation(backend, sources, tmp_path, monkeypatch):
    monkeypatch.setattr(cli, "PAIR_CHUNK_READS", 300)
    grouped = []
    add = F.Collapse.add

    def spy_add(self, *a, **k):
        grouped.append(k.get("hash") is not None and k.get("rep") is not None)
        return add(self, *a, **k)
    monkeypatch.setattr(F.Collapse, "add", spy_add)
    off, log0, seen0 = run_cli(backend, tmp_path, "off", sources["forward"], sources["reverse"], collapse=True)
    assert seen0 == [] and grouped == [False] * 4
    del grouped[:]
    on, log, seen = run_cli(backend, tmp_path, "on", sources["forward"], sources["reverse"], collapse=True, device_collapse=True)
    assert off.keys() == on.keys() and len(on) >= 4 and off == on
    assert "does not apply" not in log and "--device_collapse" not in log, log
    assert grouped == [True] * 4 and [s[0] for s in seen] == ["collapse_text"] * 4 and all(s[2] > 0 for s in seen)
    from test_cli_golden import same_files
    same_files(str(tmp_path / "on"), "paired")


def test_single_end_usearch_goes_through_the_ee_capable_call(backend, sources, tmp_path):
    for i, kw in enumerate((dict(), dict(output_format="fastq", truncate=100, relabel="Seq"))):
        off, _, seen0 = run_cli(backend, tmp_path, "off%d" % i, sources["forward"], collapse=False, pipeline="USEARCH", **kw)
        on, log, seen = run_cli(backend, tmp_path, "on%d" % i, sources["forward"], collapse=False, pipeline="USEARCH", device_format=True, **kw)
        assert seen0 == [] and off.keys() == on.keys() and len(on) >= 2 and off == on
        assert "does not apply" not in log and "--device_format" not in log, log
        assert seen and all(s[0] == "format_text" and s[4] and s[2] > 0 for s in seen)
        assert any(b";ee=" in v and b";size=1;" in v for v in on.values())


def test_a_chunk_with_a_handed_back_pair_goes_the_host_way_said_once(backend, sources, tmp_path, monkeypatch):
    monkeypatch.setattr(cli, "PAIR_CHUNK_READS", 300)
    for i, (kw, switch) in enumerate(((dict(collapse=False), "device_format"), (dict(collapse=True), "device_collapse"))):
        off, _, _ = run_cli(backend, tmp_path, "off%d" % i, sources["forward_385"], sources["reverse"], **kw)
        on, log, seen = run_cli(backend, tmp_path, "on%d" % i, sources["forward_385"], sources["reverse"], **dict(kw, **{switch: True}))
        assert off.keys() == on.keys() and off == on
        said = [l for l in log.splitlines() if l.startswith("--%s: a chunk was not" % switch)]
        assert len(said) == 1 and "it came the host way" in said[0], log
        assert len({s[2] for s in seen}) == 3 and all(s[2] > 0 for s in seen)      # the three other chunks came from the device
