"""The CPU half of --device_inflate: fastio.GzipReader with an inflater handed in (a fake one: Python's zlib, which marks chosen
members done = 0, or raises), the host decoder's error on a corrupt member word for word, the owner of the run's auxiliary
engine (one engine, one lock, each role's message once), the switches where they do not apply, and the restart on the line
parser.  The kernel: tests/test_gpu_bgzf_inflate.py; its lane code:
tests/test_inflate_lane_model.py."""
import gzip
import io
import os
import zlib

import numpy as np
import pytest

from helpers import inflate_inputs as I
from moira_amd import cli
from moira_amd import fastio as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


class FakeInflater:
    """zlib on every member; `hand_back(k, member bytes)`: leave that member to the host (done = 0, its bytes untouched);
    `refuse`: raise instead.  Remembers its calls and reports."""

    def __init__(self, hand_back=lambda k, m: False, refuse=False):
        self.hand_back, self.refuse, self.calls, self.members, self.reports = hand_back, refuse, 0, 0, []

    def __call__(self, data, offs, sizes, out_offs, out):
        self.calls += 1
        if self.refuse:
            raise RuntimeError("HIP error: planted")
        done = np.zeros(len(offs), np.uint8)
        for k in range(len(offs)):
            m = bytes(data[int(offs[k]):int(offs[k]) + int(sizes[k])])
            off, slen, crc, isize = I.parse(m)
            if self.hand_back(self.members + k, m):
                continue
            try:
                text = zlib.decompress(m[off:off + slen], -15)
            except zlib.error:
                continue
            if len(text) == isize == int(out_offs[k + 1] - out_offs[k]) and zlib.crc32(text) == crc:
                out[int(out_offs[k]):int(out_offs[k + 1])] = np.frombuffer(text, np.uint8)
                done[k] = 1
        self.members += len(offs)
        return done

    def report(self, e):
        self.reports.append(str(e))


def read_all(blob, request=1 << 22, **kw):
    r = F.GzipReader(io.BytesIO(blob), **kw)
    parts = []
    while True:
        d = r.read(request)
        if not d:
            break
        parts.append(d)
    return b"".join(parts), r


@pytest.fixture(scope="module")
def bgzf_golden():
    text = gzip.open(os.path.join(GOLD, "test1.fastq.gz")).read()
    return cli.bgzf_compress(text, 4) + cli.BGZF_EOF, text


@pytest.mark.parametrize("threads", [1, 4])
@pytest.mark.parametrize("request_bytes", [1 << 22, 100000])
def test_text_equals_the_plain_readers(bgzf_golden, threads, request_bytes):
    blob, text = bgzf_golden
    plain, _ = read_all(blob, request_bytes, threads=4)
    assert plain == text
    fi = FakeInflater()
    got, r = read_all(blob, request_bytes, threads=threads, inflater=fi)
    assert got == text and fi.calls >= 1 and r.bgzf_batches == fi.calls
    assert r.inflater_members == fi.members > len(text) // 65280 and r.inflater_handed_back == 0
    # members the inflater leaves are decoded by the host, each into its place
    fi = FakeInflater(hand_back=lambda k, m: k % 3 != 1)
    got, r = read_all(blob, request_bytes, threads=threads, inflater=fi)
    assert got == text and 0 < r.inflater_handed_back < r.inflater_members
    fi = FakeInflater(hand_back=lambda k, m: True)
    got, r = read_all(blob, request_bytes, threads=threads, inflater=fi)
    assert got == text and r.inflater_handed_back == r.inflater_members


def test_zero_padding_end_marker_and_plain_gzip_are_untouched(bgzf_golden):
    blob, text = bgzf_golden
    fi = FakeInflater()
    assert read_all(blob + b"\0" * 100, inflater=fi)[0] == text
    assert read_all(blob[:-len(cli.BGZF_EOF)], inflater=fi)[0] == text          # no end marker
    # a plain gzip file: the one-stream decoder takes it, the inflater is never called
    fi = FakeInflater()
    plain = open(os.path.join(GOLD, "test1.fastq.gz"), "rb").read()
    assert read_all(plain, inflater=fi)[0] == text and fi.calls == 0
    # BGZF members, then a plain member: the inflater sees the first part only
    fi = FakeInflater()
    got, r = read_all(blob[:-len(cli.BGZF_EOF)] + gzip.compress(b"tail\n"), inflater=fi)
    assert got == text + b"tail\n" and fi.calls >= 1


@pytest.mark.parametrize("name", ["wrong_crc", "distance_before_start", "final_block_one_short", "cut_mid_symbol"])
def test_a_corrupt_member_raises_the_hosts_error_word_for_word(bgzf_golden, name):
    blob, text = bgzf_golden
    bad = next(m for n, m, _ in I.crafted_invalid() if n == name)
    members = [cli.bgzf_compress(text[:70000], 4), bad, cli.bgzf_compress(text[70000:90000], 4), bad]     # 2 members, bad, 1, bad
    data = b"".join(members) + cli.BGZF_EOF
    with pytest.raises(OSError) as host:
        read_all(data, threads=4)
    assert "BGZF block 2:" in str(host.value)
    for fi in (FakeInflater(), FakeInflater(hand_back=lambda k, m: True), FakeInflater(refuse=True)):
        with pytest.raises(OSError) as e:
            read_all(data, threads=4, inflater=fi)
        assert str(e.value) == str(host.value)


def test_an_inflater_that_raises_sends_the_batch_to_the_host_and_is_told(bgzf_golden):
    blob, text = bgzf_golden
    fi = FakeInflater(refuse=True)
    got, r = read_all(blob, 100000, threads=2, inflater=fi)
    assert got == text and fi.calls == r.bgzf_batches > 1 and len(fi.reports) == fi.calls and "planted" in fi.reports[0]
    assert r.inflater_members == 0


class FakeEngine:
    """What the run's auxiliary engine is asked, and whether the owner's lock was held while it was."""
    made = []

    def __init__(self, device):
        self.device, self.calls, self.closed, self.owner = device, [], 0, None
        FakeEngine.made.append(self)

    def bgzf_compress(self, data):
        self.calls.append(("compress", data, self.owner.lock.locked()))
        return b"members"

    def bgzf_inflate(self, data, offs, sizes, out_offs, out=None):
        self.calls.append(("inflate", (data, offs, sizes, out_offs, out), self.owner.lock.locked()))
        return out, "done"

    def close(self):
        self.closed += 1


def test_the_runs_two_roles_share_one_engine_under_one_lock_and_each_reports_once():
    FakeEngine.made.clear()
    said = []
    d = cli._DevicePaths({"device_compress", "device_inflate"}, 3, said.append, make=FakeEngine)
    fake, = FakeEngine.made                                  # one engine for the two roles, on the device it was told
    fake.owner = d
    assert fake.device == 3 and not d.pack and not d.contigs
    assert d.compressor.compress(b"text") == b"members" and d.inflater("d", "o", "s", "oo", "out") == "done"
    assert fake.calls == [("compress", b"text", True), ("inflate", ("d", "o", "s", "oo", "out"), True)] and not d.lock.locked()
    d.compressor.report(RuntimeError("a")); d.compressor.report(RuntimeError("b"))
    d.inflater.report(RuntimeError("c")); d.inflater.report(RuntimeError("d"))
    assert len(said) == 2
    assert "--device_compress" in said[0] and "(a)" in said[0] and "host zlib" in said[0]
    assert "--device_inflate" in said[1] and "(c)" in said[1] and "host inflater" in said[1]
    d.close()
    assert fake.closed == 1
    d.close()                                                # a second close does nothing
    assert fake.closed == 1 and len(FakeEngine.made) == 1
    # say=None (--nowarnings): nothing is said; one role alone has its engine too, and no switch has none
    for on, n in (({"device_compress", "device_inflate"}, 1), ({"device_inflate"}, 1), ({"device_pack", "device_contigs"}, 0)):
        FakeEngine.made.clear()
        q = cli._DevicePaths(on, 0, None, make=FakeEngine)
        assert (q.compressor is not None) == ("device_compress" in on) and (q.inflater is not None) == ("device_inflate" in on)
        for role in (q.compressor, q.inflater):
            if role is not None:
                role.report(RuntimeError("x"))
        q.pack_refused(ValueError("x"))
        q.close(); q.close()
        assert len(FakeEngine.made) == n and all(e.closed == 1 for e in FakeEngine.made)
    assert len(said) == 2


def run_cli(tmp_path, name, oracle, source, **kw):
    from test_cli_golden import oracle_backend, reference_args
    out = str(tmp_path / name)
    a = reference_args(paired=False, forward_fastq=source, output_prefix=out, silent=True, **kw)
    log = io.StringIO()
    assert cli.main(a, backend=oracle_backend(oracle), out=log) == 0
    files = sorted(p for p in os.listdir(str(tmp_path)) if p.startswith(name + "."))
    return {p.split(".", 1)[1]: open(os.path.join(str(tmp_path), p), "rb").read() for p in files}, log.getvalue()


def test_the_switch_without_a_gpu_says_so_once_and_changes_no_file(tmp_path, oracle, bgzf_golden):
    src = str(tmp_path / "in.fastq.gz")
    with open(src, "wb") as f:
        f.write(bgzf_golden[0])
    off, log_off = run_cli(tmp_path, "off", oracle, src)
    on, log_on = run_cli(tmp_path, "on", oracle, src, device_inflate=True)
    assert "--device_inflate" not in log_off
    assert log_on.count("--device_inflate does not apply to this run") == 1 and "the host inflater is used" in log_on
    assert off.keys() == on.keys() and len(off) >= 3 and off == on
    quiet, log_quiet = run_cli(tmp_path, "quiet", oracle, src, device_inflate=True, nowarnings=True)
    assert "--device_inflate" not in log_quiet and quiet == off


def test_both_auxiliary_switches_without_a_gpu_say_so_in_order_and_leave_args_alone(tmp_path, oracle, bgzf_golden):
    from test_cli_golden import oracle_backend, reference_args
    src = str(tmp_path / "in.fastq.gz")
    with open(src, "wb") as f:
        f.write(bgzf_golden[0])
    off, _ = run_cli(tmp_path, "off", oracle, src, output_compression="gz")
    a = reference_args(paired=False, forward_fastq=src, output_prefix=str(tmp_path / "on"), silent=True, output_compression="gz",
                       device_inflate=True, device_compress=True)
    names = sorted(vars(a))
    log = io.StringIO()
    assert cli.main(a, backend=oracle_backend(oracle), out=log) == 0
    assert sorted(vars(a)) == names                              # nothing is written onto the parsed arguments
    lines = [l for l in log.getvalue().splitlines() if "does not apply to this run" in l]
    assert [l.split(" ")[0] for l in lines] == ["--device_compress", "--device_inflate"]
    assert "host zlib is used." in lines[0] and "the host inflater is used." in lines[1]
    on = {p.split(".", 1)[1]: open(os.path.join(str(tmp_path), p), "rb").read() for p in sorted(os.listdir(str(tmp_path))) if p.startswith("on.")}
    assert off.keys() == on.keys() and len(off) >= 3 and off == on


def test_the_restart_on_the_line_parser_closes_first_and_says_what_a_second_run_says(tmp_path, oracle, monkeypatch):
    """Old-Mac line ends make the byte-level parser raise fastio.Unsupported: the run starts over on the line parser, where no
    device path applies, so the `--device_pack does not apply` line is said by the first pass (no device) and by the second."""
    from test_cli_golden import oracle_backend, reference_args
    from test_fastio import make_fastq, outputs_of
    src = tmp_path / "cr.fastq"
    src.write_bytes(make_fastq(np.random.default_rng(1), 40, quirks=False).replace("\n", "\r").encode())
    runs = []
    real = cli._run_fast_fastq
    monkeypatch.setattr(cli, "_run_fast_fastq", lambda *a, **k: (runs.append(1), real(*a, **k))[1])
    log = io.StringIO()
    a = reference_args(paired=False, collapse=False, forward_fastq=str(src), output_prefix=str(tmp_path / "a"), device_pack=True)
    assert cli.main(a, backend=oracle_backend(oracle), out=log) == 0
    assert runs == [1]                                           # the byte-level path was tried, once
    assert log.getvalue().count("--device_pack does not apply to this run") == 2
    monkeypatch.setenv("MOIRA_NO_FASTIO", "1")
    b = reference_args(paired=False, collapse=False, forward_fastq=str(src), output_prefix=str(tmp_path / "b"))
    assert cli.main(b, backend=oracle_backend(oracle), out=open(os.devnull, "w")) == 0
    got, want = outputs_of(str(tmp_path / "a")), outputs_of(str(tmp_path / "b"))
    assert got == want and sum(len(v) for v in got.values()) > 100


def test_the_parser_knows_the_switch_and_it_is_off_by_default():
    p = cli.build_parser()
    assert p.parse_args(["-ffq", "x"]).device_inflate is False
    assert p.parse_args(["-ffq", "x", "--device_inflate"]).device_inflate is True
    assert "--device_inflate" in p.format_help()
