"""The CLI on reads of up to 65535 bases with every opt-in device path of the text side on (--device_index --device_pack
--device_format --device_collapse; --device_fasta_qual for the fasta+qual rendering) against none of them: every output file
must be byte-equal.  The input is tests/helpers/long_read_inputs.py's records plus 200 golden reads; with blocks of 50,000 bytes
a record of 131 KB is carried over whole blocks that complete no record.  A file whose third record has 65536 bases ends in the
same ReadTooLongError text and exit status either way.  The runs share one backend in this process, as
tests/test_gpu_collapse_cli.py's and tests/test_gpu_fasta_qual_cli.py's do.  The entries themselves: tests/test_gpu_long_text.py."""
import io
import os

import pytest

from helpers import bgzf_fastq_inputs
from helpers import fasta_qual_inputs
from helpers import long_read_inputs as X
from moira_amd import cli
from moira_amd import fastio as F

pytestmark = pytest.mark.gpu

SWITCHES = dict(device_index=True, device_pack=True, device_format=True, device_collapse=True)
FLAGS = [dict(collapse=True), dict(collapse=False), dict(collapse=False, output_format="fastq", truncate=40000)]
FLAG_IDS = ["collapse", "format_fasta_qual", "format_fastq_truncate_40000"]


@pytest.fixture(scope="module")
def backend():
    be = cli.make_gpu_backend(None)
    yield be
    be.engine.close()


@pytest.fixture(scope="module")
def sources(tmp_path_factory):
    """The long records and 200 golden reads as a FASTQ file and as a fasta + qual pair; a FASTQ and a fasta + qual pair whose
    third record has 65536 bases."""
    d = tmp_path_factory.mktemp("long_inputs")
    text = X.fastq_text()[0] + bgzf_fastq_inputs.golden_text(200)
    idx = F.index(text, True, 1000)[0]
    assert len(idx) == len(X.LENGTHS) + 200
    recs = [(text[int(r[F.HDR_OFF]):int(r[F.HDR_OFF] + r[F.HDR_LEN])], text[int(r[F.SEQ_OFF]):int(r[F.SEQ_OFF] + r[F.SEQ_LEN])],
             [X._TOK[v - 33] for v in text[int(r[F.QUAL_OFF]):int(r[F.QUAL_OFF] + r[F.QUAL_LEN])]]) for r in idx]
    f, q = fasta_qual_inputs.render(recs)
    long_text, lidx = X.too_long_text()
    lrecs = [(b"long%d" % k, long_text[int(r[F.SEQ_OFF]):int(r[F.SEQ_OFF] + r[F.SEQ_LEN])],
              [X._TOK[v - 33] for v in long_text[int(r[F.QUAL_OFF]):int(r[F.QUAL_OFF] + r[F.QUAL_LEN])]]) for k, r in enumerate(lidx)]
    lf, lq = fasta_qual_inputs.render(lrecs)
    for name, data in (("long.fastq", text), ("long.fasta", f), ("long.qual", q), ("too_long.fastq", long_text), ("too_long.fasta", lf),
                       ("too_long.qual", lq)):
        (d / name).write_bytes(data)
    return {k: str(d / k) for k in ("long.fastq", "long.fasta", "long.qual", "too_long.fastq", "too_long.fasta", "too_long.qual")}


def files_of(tmp_path, name):
    return {p.split(".", 1)[1]: open(os.path.join(str(tmp_path), p), "rb").read() for p in sorted(os.listdir(str(tmp_path)))
            if p.startswith(name + ".")}


def run_cli(backend, tmp_path, name, **kw):
    """-> (exit status, the files, the log, the records of the engine's fused filter calls)."""
    from test_cli_golden import reference_args
    a = reference_args(paired=False, output_prefix=str(tmp_path / name), error_calc="poisson_binomial", **kw)
    eng, seen = backend.engine, []
    inner = eng.filter_fastq, eng.filter_fasta_qual

    def watch(call):
        def f(*x, **k):
            r = call(*x, **k)
            seen.append(len(r.idx))
            return r
        return f
    eng.filter_fastq, eng.filter_fasta_qual = watch(inner[0]), watch(inner[1])
    log = io.StringIO()
    try:
        rc = cli.main(a, backend=backend, out=log)
    finally:
        eng.filter_fastq, eng.filter_fasta_qual = inner
    return rc, files_of(tmp_path, name), log.getvalue(), seen


@pytest.mark.parametrize("flags", FLAGS, ids=FLAG_IDS)
def test_long_fastq_records_come_out_the_same_with_every_device_path_on(backend, sources, tmp_path, monkeypatch, flags):
    n = len(X.LENGTHS) + 200
    rc, off, _, seen = run_cli(backend, tmp_path, "off", forward_fastq=sources["long.fastq"], **flags)
    assert rc == 0 and seen == [] and len(off) >= 2 and sum(len(v) for v in off.values()) > 500000
    rc, on, log, seen = run_cli(backend, tmp_path, "on", forward_fastq=sources["long.fastq"], **dict(flags, **SWITCHES))
    assert rc == 0 and on == off and sum(seen) == n
    assert "did not take" not in log and "host way" not in log, log
    if flags["collapse"]:                                    # blocks of 50,000 bytes: a 131 KB record waits over two whole blocks
        monkeypatch.setattr(cli, "DEVICE_INDEX_BLOCK", 50000)
        rc, small, log, seen = run_cli(backend, tmp_path, "small", forward_fastq=sources["long.fastq"], **dict(flags, **SWITCHES))
        assert rc == 0 and small == off and sum(seen) == n and "did not take" not in log
        assert len(seen) >= 12 and [a == b == 0 for a, b in zip(seen, seen[1:])].count(True) >= 1      # two calls in a row complete no record


@pytest.mark.parametrize("flags", FLAGS, ids=FLAG_IDS)
def test_long_fasta_qual_records_come_out_the_same_with_the_switch(backend, sources, tmp_path, flags):
    n = len(X.LENGTHS) + 200
    src = dict(forward_fasta=sources["long.fasta"], forward_qual=sources["long.qual"])
    rc, off, _, seen = run_cli(backend, tmp_path, "off", **src, **flags)
    assert rc == 0 and seen == [] and len(off) >= 2 and sum(len(v) for v in off.values()) > 500000
    more = dict(device_fasta_qual=True, device_format=True, device_collapse=True)
    rc, on, log, seen = run_cli(backend, tmp_path, "on", **src, **dict(flags, **more))
    assert rc == 0 and on == off and sum(seen) == n and "did not take" not in log, log


def test_a_third_record_of_65536_bases_ends_the_run_the_same_way(backend, sources, tmp_path):
    ends = []
    for src, more in ((dict(forward_fastq=sources["too_long.fastq"]), SWITCHES),
                      (dict(forward_fasta=sources["too_long.fasta"], forward_qual=sources["too_long.qual"]),
                       dict(device_fasta_qual=True, device_format=True, device_collapse=True))):
        rc, off, log_off, _ = run_cli(backend, tmp_path, "off", collapse=False, silent=False, **src)
        rc_on, on, log_on, _ = run_cli(backend, tmp_path, "on", collapse=False, silent=False, **dict(src, **more))
        told = [ln for ln in log_off.splitlines() if "65536 bases" in ln]
        assert rc == rc_on == 1 and len(told) == 1 and told[0].startswith("Sequence long2 has 65536 bases") and "65535" in told[0]
        assert told == [ln for ln in log_on.splitlines() if "65536 bases" in ln]       # (the ReadTooLongError's text)
        if "forward_fastq" in src:                           # the index's block is handed back first and says so, once
            assert log_on.count("--device_index: the device did not take a block (reads longer than 65535 bases") == 1
        assert on == off                                     # (what the records before it had written is removed in both runs)
        ends.append(told[0])
    assert ends[0] == ends[1]
