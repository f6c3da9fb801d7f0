"""The CLI with --device_fasta_qual on the GPU.  The single-end fasta+qual cases of tests/golden/flag_matrix (fa_se_*) run with
the switch and must reproduce the reference's files byte for byte: their input holds scores of 120 and 300, so the block with
the 300 is handed back, the host function calls it unsupported as well, and the run ends in the reference's output through the
line parser, as it does without the switch -- with one line that says so.  The golden reads rendered to fasta+qual without
such scores go through the device whole: with tiny blocks (one file starves, records are carried), with --device_format
(-c false) and with --device_collapse (-c true); every output file must be byte-equal to the run without the switch.  The
matrix runs in this process on one backend; one run goes through moira.py as a command, under its own timeout.  The entries
themselves: tests/test_gpu_fasta_qual.py."""
import io
import os
import subprocess
import sys

import pytest

from helpers import bgzf_inputs
from moira_amd import cli
from test_flag_matrix import MAN, _args, expected, inputs      # noqa: F401 -- the two fixtures

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FA_SE = sorted(c for c in MAN["cases"] if c.startswith("fa_se_"))
HANDED_BACK = "--device_fasta_qual: the device did not take a block (quality token): the host parser is used for it."


@pytest.fixture(scope="module")
def backend():
    be = cli.make_gpu_backend(None)
    yield be
    be.engine.close()


@pytest.fixture(scope="module")
def clean(tmp_path_factory):
    """The golden reads as fasta + qual files that the byte-level path takes whole."""
    d = tmp_path_factory.mktemp("fasta_qual_inputs")
    _, f, q = bgzf_inputs.golden_renderings()
    (d / "golden.fasta").write_bytes(f), (d / "golden.qual").write_bytes(q)
    return str(d / "golden.fasta"), str(d / "golden.qual")


def files_of(tmp_path, name):
    return {p.split(".", 1)[1]: open(os.path.join(str(tmp_path), p), "rb").read() for p in sorted(os.listdir(str(tmp_path)))
            if p.startswith(name + ".")}


def run_cli(backend, tmp_path, name, src, flags=None, **kw):
    """-> (the files; the log; what the engine's three calls saw: records per filter_fasta_qual / format_text / collapse_text call)."""
    a = _args(dict(flags or {}), forward_fasta=src[0], forward_qual=src[1], output_prefix=str(tmp_path / name), **kw)
    seen = dict(filter=[], format=[], collapse=[])
    eng = backend.engine
    inner = eng.filter_fasta_qual, eng.format_text, eng.collapse_text

    def filter_fasta_qual(*x, **k):
        r = inner[0](*x, **k)
        seen["filter"].append(len(r.idx))
        return r

    def format_text(*x, **k):
        seen["format"].append(len(k["sel"]))
        return inner[1](*x, **k)

    def collapse_text(*x, **k):
        seen["collapse"].append(k["n"])
        return inner[2](*x, **k)
    eng.filter_fasta_qual, eng.format_text, eng.collapse_text = filter_fasta_qual, format_text, collapse_text
    log = io.StringIO()
    try:
        assert cli.main(a, backend=backend, out=log) == 0
    finally:
        eng.filter_fasta_qual, eng.format_text, eng.collapse_text = inner
    return files_of(tmp_path, name), log.getvalue(), seen


@pytest.mark.parametrize("case", FA_SE)
def test_the_flag_matrix_cases_come_out_as_the_reference_wrote_them(case, inputs, expected, tmp_path, backend):
    assert len(FA_SE) == 3
    spec = MAN["cases"][case]
    got, log, seen = run_cli(backend, tmp_path, "o", inputs[spec["input"]][0], spec["flags"], device_fasta_qual=True)
    assert got == expected[case] and sorted(got) == sorted(spec["files"])
    # the score of 300: handed back, said once, and the line parser's output all the same
    assert log.count(HANDED_BACK) == 1 and log.count("--device_fasta_qual") == 2 and log.count(cli.DEVICE_FASTA_QUAL_SENTENCE) == 1, log


def test_tiny_blocks_starve_one_file_and_end_in_the_same_files(inputs, expected, tmp_path, backend, monkeypatch):
    monkeypatch.setattr(cli, "FASTA_QUAL_BLOCKS", (1500, 900))
    case = "fa_se_default"
    got, log, seen = run_cli(backend, tmp_path, "o", inputs[MAN["cases"][case]["input"]][0], device_fasta_qual=True)
    assert got == expected[case] and log.count(HANDED_BACK) == 1
    assert len(seen["filter"]) >= 2 and 0 < sum(seen["filter"]) < 1040                           # chunks came from the device before the 300


@pytest.mark.parametrize("flags", [dict(), dict(collapse=False), dict(collapse=False, truncate=100, output_format="fastq"),
                                   dict(truncate=150, error_calc="poisson")], ids=["default", "nocollapse", "fastq_t100", "poisson_t150"])
def test_clean_reads_go_through_the_device_whole_and_the_files_are_identical(clean, tmp_path, backend, flags, monkeypatch):
    off, _, seen = run_cli(backend, tmp_path, "off", clean, flags)
    assert seen["filter"] == [] and len(off) >= 2
    on, log, seen = run_cli(backend, tmp_path, "on", clean, flags, device_fasta_qual=True)
    assert on == off and "--device_fasta_qual" not in log, log
    assert seen["filter"] == [1000] and seen["format"] == seen["collapse"] == []
    monkeypatch.setattr(cli, "FASTA_QUAL_BLOCKS", (20000, 500))             # (a qual block holds less than a record: most calls starve)
    tiny, log, seen = run_cli(backend, tmp_path, "tiny", clean, flags, device_fasta_qual=True, processors=16)
    assert tiny == off and "--device_fasta_qual" not in log, log
    assert sum(seen["filter"]) == 1000 and len(seen["filter"]) > 10 and 0 in seen["filter"]


def test_device_format_goes_on_from_the_chunk_the_switch_leaves(clean, tmp_path, backend, monkeypatch):
    monkeypatch.setattr(cli, "FASTA_QUAL_BLOCKS", (100000, 300000))
    for name, flags in (("fa", dict(collapse=False)), ("fq", dict(collapse=False, output_format="fastq", truncate=100))):
        off, _, _ = run_cli(backend, tmp_path, name + "_off", clean, flags)
        on, log, seen = run_cli(backend, tmp_path, name + "_on", clean, flags, device_fasta_qual=True, device_format=True)
        assert on == off and "--device_f" not in log, log
        assert len(seen["filter"]) >= 3 and sum(seen["format"]) == (1 if "output_format" in flags else 2) * 1000 and seen["collapse"] == []
    # with -c true the format switch says its sentence, and the files are what they were
    off, _, _ = run_cli(backend, tmp_path, "c_off", clean)
    on, log, seen = run_cli(backend, tmp_path, "c_on", clean, device_fasta_qual=True, device_format=True)
    assert on == off and log.count(cli.DEVICE_FORMAT_SENTENCE) == 1 and seen["format"] == []


def test_device_collapse_goes_on_from_the_chunk_the_switch_leaves(clean, tmp_path, backend, monkeypatch):
    monkeypatch.setattr(cli, "FASTA_QUAL_BLOCKS", (100000, 300000))
    for name, flags in (("c", dict()), ("ct", dict(truncate=100))):
        off, _, _ = run_cli(backend, tmp_path, name + "_off", clean, flags)
        on, log, seen = run_cli(backend, tmp_path, name + "_on", clean, flags, device_fasta_qual=True, device_collapse=True, processors=16)
        assert on == off and "--device_" not in log, log
        assert len(seen["filter"]) >= 3 and sum(seen["collapse"]) == 1000 and seen["format"] == []


def test_the_command_line_takes_the_switch(clean, tmp_path):
    base = [sys.executable, os.path.join(ROOT, "moira.py"), "-ff", clean[0], "-fq", clean[1], "--silent", "-p", "16"]
    for name, more in (("off", []), ("on", ["--device_fasta_qual", "--device_collapse"])):
        p = subprocess.run(base + ["-op", str(tmp_path / name)] + more, capture_output=True, text=True, cwd=ROOT, timeout=300)
        assert p.returncode == 0 and "--device_" not in p.stdout + p.stderr, p.stdout[-2000:] + p.stderr[-2000:]
    assert files_of(tmp_path, "on") == files_of(tmp_path, "off") and len(files_of(tmp_path, "on")) == 6
