"""k_bgzf_inflate on the GPU (include/moira_pb.h: mpb_bgzf_inflate_host; Engine.bgzf_inflate; fastio.GzipReader's inflater; the CLI's
--device_inflate).  The yardstick is the host decoder, libmoira_io's mio_bgzf_inflate_mt: every valid input comes back as its
text with every member taken and consistent counts; every invalid member, between two valid ones, is handed back with its reason
while its neighbours are taken; what the host rejects is never taken.  The lane code on the CPU: tests/test_inflate_lane_model.py;
the rows: tests/test_bgzf_member_rows.py; the reader and the switch without a GPU: tests/test_device_inflate_reader.py."""
import gzip
import io
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import bgzf_inputs as B
from helpers import inflate_inputs as I
from moira_amd import cli
from moira_amd import engine as E
from moira_amd import fastio as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(0)
    yield e
    e.close()


def host_text(members):
    """The members' text by mio_bgzf_inflate_mt, all in one call."""
    blob, offs, sizes, out_offs = I.layout(members)
    out = np.zeros(max(int(out_offs[-1]), 1), np.uint8)
    buf = np.frombuffer(blob + b"\0" * 8, np.uint8)
    rc = F.load().mio_bgzf_inflate_mt(buf.ctypes.data, offs.ctypes.data, sizes.ctypes.data, out_offs.ctypes.data, len(members),
                                      out.ctypes.data, 4)
    assert rc == 0, F.load().mio_inflate_error()
    return out[:int(out_offs[-1])].tobytes()


def inflate(eng, members):
    blob, offs, sizes, out_offs = I.layout(members)
    text, done, why = eng.bgzf_inflate(blob, offs, sizes, out_offs)
    return text.tobytes(), done, why, dict(eng.bgzf_inflate_stats()), out_offs


def split_members(blob):
    ends = np.cumsum([bsize + 1 for bsize, _, _, _ in B.split_bgzf(blob)]).tolist()
    return [blob[a:b] for a, b in zip([0] + ends[:-1], ends)]


def check_valid(eng, cases):
    members = [I.frame(s, t) for _, s, t, _ in cases]
    text, done, why, st, out_offs = inflate(eng, members)
    assert done.tolist() == [1] * len(cases), [(c[0], int(w)) for c, d, w in zip(cases, done, why) if not d]
    assert not why.any()
    assert text == host_text(members) == b"".join(t for _, _, t, _ in cases)
    assert st["members"] == st["taken"] == len(cases) and st["handed_back"] == 0
    return st


@pytest.mark.parametrize("name", [c[0] for c in I.crafted_valid() + I.zlib_members()])
def test_valid_member(eng, name):
    case = next(c for c in I.crafted_valid() + I.zlib_members() if c[0] == name)
    st = check_valid(eng, [case])
    _, _, text, blocks = case
    stored_bytes = len(text) - st["literals"] - st["matched_bytes"]      # literals + matched bytes + stored bytes = text bytes
    assert stored_bytes >= 0 and (st["stored_blocks"] > 0 or stored_bytes == 0)
    if blocks is not None:
        assert (st["stored_blocks"], st["fixed_blocks"], st["dynamic_blocks"]) == blocks
    if name in ("fibonacci", "dist_ladder_15bit"):
        assert st["longest_code"] == 15
    if name == "memlevel1":
        assert st["dynamic_blocks"] > 30
    if name == "level0":
        assert stored_bytes == len(text)
    if name == "rle":
        assert st["matches"] > 0


def test_all_valid_members_in_one_call_and_again(eng):
    cases = I.crafted_valid() + I.zlib_members()
    st = check_valid(eng, cases)
    assert st["longest_code"] == 15
    assert check_valid(eng, cases) == st                      # a second call gives equal results


@pytest.mark.parametrize("name", [c[0] for c in I.crafted_invalid()])
def test_invalid_member_between_two_valid_ones(eng, name):
    _, bad, reason = next(c for c in I.crafted_invalid() if c[0] == name)
    good, good_text = I.neighbour()
    members = [good, bad, good]
    htext, herr = I.host_inflate([bad])[0]
    text, done, why, st, out_offs = inflate(eng, members)
    assert done.tolist() == [1, 0, 1] and why.tolist() == [I.OK, reason, I.OK]
    assert text[:len(good_text)] == good_text and text[int(out_offs[2]):] == good_text
    assert (st["taken"], st["handed_back"]) == (2, 1)
    assert herr is not None or reason == I.HEADER             # (the one member the host takes: plain gzip, no 'B','C')


def test_damaged_members_are_taken_only_with_the_hosts_bytes(eng):
    rng = np.random.default_rng(78)
    base = [c for c in I.zlib_members() if len(c[1]) < 12000][:5] + I.crafted_valid()[:4]
    members = []
    for _, stream, text, _ in base:
        for _ in range(8):
            s = bytearray(stream)
            if rng.random() < 0.3:
                s = s[:int(rng.integers(1, len(s)))]
            else:
                s[int(rng.integers(0, len(s)))] ^= 1 << int(rng.integers(0, 8))
            members.append(I.frame(bytes(s), text))
    text, done, why, st, out_offs = inflate(eng, members)
    host = I.host_inflate(members)
    assert 0 < st["handed_back"] == len(members) - int(done.sum())
    for k, (htext, herr) in enumerate(host):
        if done[k]:
            assert htext is not None and text[int(out_offs[k]):int(out_offs[k + 1])] == htext
        else:
            assert why[k] != I.OK


@pytest.mark.parametrize("piece", [1, 3])
def test_piece_loop(eng, piece, monkeypatch):
    cases = (I.crafted_valid() + I.zlib_members()[:3])[:7]
    assert len(cases) == 7
    whole = check_valid(eng, cases)
    monkeypatch.setenv("MPB_BGZF_INFLATE_PIECE_MEMBERS", str(piece))
    assert check_valid(eng, cases) == whole
    # a handed-back member in the middle of a piece loop
    _, bad, reason = next(c for c in I.crafted_invalid() if c[0] == "trailing_byte")
    members = [I.frame(s, t) for _, s, t, _ in cases]
    members.insert(4, bad)
    text, done, why, st, out_offs = inflate(eng, members)
    assert done.tolist() == [1, 1, 1, 1, 0, 1, 1, 1] and why[4] == reason
    want = host_text(members[:4]) + b"\0" * int(out_offs[5] - out_offs[4]) + host_text(members[5:])
    assert text[:int(out_offs[4])] == want[:int(out_offs[4])] and text[int(out_offs[5]):] == want[int(out_offs[5]):]


def test_fuzz_members(eng):
    st = check_valid(eng, I.fuzz_members())
    assert st["members"] == 24


def test_device_written_members_round_trip(eng):
    for text in B.golden_renderings():
        blob = eng.bgzf_compress(text)
        members = split_members(blob)
        got, done, why, st, _ = inflate(eng, members)
        assert got == text and done.all() and st["handed_back"] == 0
    # a text whose members the device stores, and one it codes with the fixed code
    for text in (np.random.default_rng(5).integers(0, 256, B.DATA + 100).astype(np.uint8).tobytes(), b"ACGT" * 10):
        blob = eng.bgzf_compress(text)
        members = split_members(blob)
        got, done, why, st, _ = inflate(eng, members)
        assert got == text and done.all()


def test_empty_call_and_bad_arguments(eng):
    text, done, why = eng.bgzf_inflate(b"", np.empty(0, np.int64), np.empty(0, np.int32), np.zeros(1, np.int64))
    assert len(text) == len(done) == len(why) == 0 and eng.bgzf_inflate_stats()["members"] == 0
    good, _ = I.neighbour()
    blob, offs, sizes, out_offs = I.layout([good])
    with pytest.raises(ValueError):
        eng.bgzf_inflate(blob[:-1], offs, sizes, out_offs)    # the member does not lie inside the input
    with pytest.raises(ValueError):
        eng.bgzf_inflate(blob, offs, sizes, out_offs[::-1].copy())


def test_kernel_time_is_reported(eng):
    eng.timing(True)
    eng.timing_reset()
    check_valid(eng, I.crafted_valid()[:3])
    t = eng.kernel_times()
    eng.timing(False)
    assert t["bgzf_inflate"][1] == 1 and t["bgzf_inflate"][0] > 0, t


def read_all(blob, **kw):
    r = F.GzipReader(io.BytesIO(blob), **kw)
    parts = []
    while True:
        d = r.read(1 << 22)
        if not d:
            break
        parts.append(d)
    return b"".join(parts), r


def test_gzip_reader_with_the_device_inflater(eng):
    text = B.golden_text()
    blob = cli.bgzf_compress(text, 4) + cli.BGZF_EOF
    said = []
    paths = cli._DevicePaths({"device_inflate"}, 0, said.append, make=lambda device: eng)      # (never closed: the fixture's engine)
    inf = paths.inflater
    got, r = read_all(blob, threads=2, inflater=inf)
    assert got == text and r.inflater_members > len(text) // B.DATA and r.inflater_handed_back == 0 and not said
    # device-written members, and a corrupt one: the host's error, word for word
    got, r = read_all(eng.bgzf_compress(text) + cli.BGZF_EOF, threads=2, inflater=inf)
    assert got == text and r.inflater_handed_back == 0
    bad = next(m for n, m, _ in I.crafted_invalid() if n == "wrong_crc")
    data = cli.bgzf_compress(text[:70000], 4) + bad + cli.BGZF_EOF
    with pytest.raises(OSError) as host:
        read_all(data, threads=2)
    with pytest.raises(OSError) as dev:
        read_all(data, threads=2, inflater=inf)
    assert str(dev.value) == str(host.value) and "BGZF block 2: CRC check failed" in str(dev.value)
    assert paths.engine is eng and not said


@pytest.mark.parametrize("paired", [False, True], ids=["forward", "paired"])
def test_cli_on_bgzf_input_with_and_without_device_inflate(tmp_path, paired):
    from test_cli_golden import reference_args
    import bz2
    src = [str(tmp_path / "in1.fastq.gz"), str(tmp_path / "in2.fastq.gz")]
    with open(src[0], "wb") as f:
        f.write(cli.bgzf_compress(B.golden_text(), 4) + cli.BGZF_EOF)
    with open(src[1], "wb") as f:
        f.write(cli.bgzf_compress(bz2.open(os.path.join(GOLD, "test2.fastq.bz2")).read(), 4) + cli.BGZF_EOF)
    got, logs, calls = [], [], []
    for on in (False, True):
        out = str(tmp_path / ("on" if on else "off"))
        a = reference_args(paired=paired, forward_fastq=src[0], output_prefix=out, reverse_fastq=src[1] if paired else None,
                           output_compression="gz" if paired else "none", processors=4)
        a.device_inflate = on
        a.device_compress = on and paired                     # together they share one auxiliary engine
        be = cli.make_gpu_backend(None)
        log = io.StringIO()
        made, engines = [], []
        inner = cli._DevicePaths.inflate
        try:
            cli._DevicePaths.inflate = lambda self, *x: (made.append(len(x[1])), engines.append(self.engine), inner(self, *x))[2]
            assert cli.main(a, backend=be, out=log) == 0
        finally:
            cli._DevicePaths.inflate = inner
            be.engine.close()
        calls.append(sum(made))
        logs.append(log.getvalue())
        assert len({id(e) for e in engines}) <= 1
        files = sorted(p for p in os.listdir(str(tmp_path)) if p.startswith(os.path.basename(out) + "."))
        assert files
        got.append({p.split(".", 1)[1]: (gzip.decompress if p.endswith(".gz") else bytes)(open(os.path.join(str(tmp_path), p), "rb").read())
                    for p in files})
    assert got[0].keys() == got[1].keys() and got[0] == got[1] and sum(len(v) for v in got[0].values()) > 100000
    assert calls[0] == 0 and calls[1] >= (2 if paired else 1) * (len(B.golden_text()) // B.DATA)       # the members went through the device
    assert not any("--device_inflate" in l for l in logs)
