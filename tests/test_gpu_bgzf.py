"""k_bgzf_deflate, k_bgzf_scan and k_bgzf_frame on the GPU (include/moira_pb.h: mpb_bgzf_compress_host; Engine.bgzf_compress; the
CLI's --device_compress).  Every input goes through the same checks: gzip reads the output back, each member's BSIZE, CRC and
ISIZE are right and its deflate stream inflates ON ITS OWN (a member is its own window), the package's reader gives the text
back on several threads, the output fits mpb_bgzf_bound, and a second call gives the same bytes.  The lane code on the CPU:
tests/test_bgzf_lane_model.py; the writer and the switch: tests/test_bgzf_writer.py."""
import ctypes as C
import gzip
import io
import os
import zlib

import numpy as np
import pytest

from helpers import bgzf_inputs as B
from moira_amd import _lib as L
from moira_amd import cli
from moira_amd import engine as E
from moira_amd import fastio as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
NAMED = dict(B.named_inputs())


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(0)
    yield e
    e.close()


def read_back(blob, threads=4):
    r = F.GzipReader(io.BytesIO(blob), threads=threads)
    parts = []
    while True:
        d = r.read(1 << 22)
        if not d:
            break
        parts.append(d)
    return b"".join(parts), r.bgzf_batches


def compress_checked(eng, text):
    """Engine.bgzf_compress(text) with every check of the module's docstring -> (output, stats)."""
    out = eng.bgzf_compress(text)
    st = dict(eng.bgzf_stats())
    cap = C.c_int64()
    assert L.load().mpb_bgzf_bound(len(text), C.byref(cap)) == 0 and len(out) <= cap.value
    assert gzip.decompress(out + cli.BGZF_EOF) == text
    ms, parts = B.split_bgzf(out), B.members(text)
    assert len(ms) == len(parts) == st["members"] == st["dynamic"] + st["fixed"] + st["stored"]
    for (bsize, stream, crc, isize), part in zip(ms, parts):
        assert bsize == len(stream) + 25 and isize == len(part) and crc == zlib.crc32(part)
        assert B.inflate_raw(stream) == part
    assert st["literals"] + st["matched_bytes"] == len(text)
    if text:
        back, batches = read_back(out + cli.BGZF_EOF)
        assert back == text and batches >= 1                       # (mio_bgzf_scan + mio_bgzf_inflate_mt took it)
    assert eng.bgzf_compress(text) == out and eng.bgzf_stats() == st
    return out, st


@pytest.mark.parametrize("name", [n for n, _ in B.named_inputs() if n.startswith("len")])
def test_lengths_at_the_member_borders(eng, name):
    text = NAMED[name]
    out, st = compress_checked(eng, text)
    assert st["members"] == -(-len(text) // B.DATA)
    if not text:
        assert out == b"" and st == dict.fromkeys(st, 0)


def test_one_byte_over_a_whole_member(eng):
    out, st = compress_checked(eng, NAMED["one_byte_member"])
    assert st["literals"] == 1 and st["matches"] == -(-(B.DATA - 1) // 258) and len(out) < 400      # distance 1, the cap of 258


@pytest.mark.parametrize("period", [3, 64, B.STEP - 1, B.STEP + 1])
def test_periods_around_the_step(eng, period):
    text = NAMED["period%d" % period]
    out, st = compress_checked(eng, text)
    assert st["matched_bytes"] >= len(text) - 3 * max(period, B.STEP)


def test_the_largest_legal_distance_and_the_first_illegal_one(eng):
    _, st = compress_checked(eng, NAMED["period32768"])
    assert st["matched_bytes"] >= (B.DATA - 32768) // 2
    _, st = compress_checked(eng, NAMED["period32769"])
    assert st["matched_bytes"] < 3000


def test_a_repeat_across_the_member_border_is_not_matched(eng):
    text = NAMED["repeat_across_border"]
    out, st = compress_checked(eng, text)                           # (every member inflates on its own there)
    assert st["members"] == 2 and st["matched_bytes"] < 300


def test_random_bytes_come_out_stored_or_fixed(eng):
    out, st = compress_checked(eng, NAMED["random_member"])
    assert (st["members"], st["stored"]) == (1, 1) and len(out) == B.DATA + 31
    out, st = compress_checked(eng, NAMED["random_1000"])
    assert st["dynamic"] == 0 and len(out) <= 1000 + 31


def test_all_byte_values_twice_and_a_text_without_a_repeat(eng):
    _, st = compress_checked(eng, NAMED["all_bytes_twice"])
    assert st["matched_bytes"] >= 250
    out, st = compress_checked(eng, NAMED["no_repeat"])
    assert st["matches"] == 0 and st["dynamic"] == 1 and len(out) < len(NAMED["no_repeat"])        # zero distance codes
    _, st = compress_checked(eng, NAMED["min_match_at_end"])                                        # exactly one distance code
    assert (st["matches"], st["matched_bytes"], st["literals"]) == (1, 3, 703)


@pytest.mark.parametrize("which", [0, 1, 2], ids=["fastq", "fasta", "qual"])
def test_golden_texts(eng, which):
    text = B.golden_renderings()[which]
    out, st = compress_checked(eng, text)
    assert st["stored"] == 0 and len(out) < len(text)


def test_fuzz_members(eng):
    for k in range(20):
        compress_checked(eng, B.fuzz_member(k))


def test_pieces_give_the_same_bytes(eng, monkeypatch):
    """A call cut into pieces of two members (MPB_BGZF_PIECE_MEMBERS) equals the call in one piece."""
    text = B.golden_renderings()[0]
    whole = eng.bgzf_compress(text)
    monkeypatch.setenv("MPB_BGZF_PIECE_MEMBERS", "2")
    assert eng.bgzf_compress(text) == whole and eng.bgzf_stats()["members"] == -(-len(text) // B.DATA)


def test_arguments_are_validated(eng):
    lib, got = L.load(), C.c_int64(7)
    buf = np.zeros(1 << 17, np.uint8)
    assert lib.mpb_bgzf_compress_host(eng.ctx, b"abc", 3, buf.ctypes.data, 3 + 30, C.byref(got), None) == L.E_INVALID
    assert b"mpb_bgzf_bound" in lib.mpb_last_error() and got.value == 0
    assert lib.mpb_bgzf_compress_host(eng.ctx, None, 3, buf.ctypes.data, 1 << 17, C.byref(got), None) == L.E_INVALID
    assert lib.mpb_bgzf_compress_host(eng.ctx, b"abc", -1, buf.ctypes.data, 1 << 17, C.byref(got), None) == L.E_INVALID
    assert lib.mpb_bgzf_compress_host(eng.ctx, b"abc", 3, buf.ctypes.data, 1 << 17, None, None) == L.E_INVALID
    assert lib.mpb_bgzf_compress_host(None, b"abc", 3, buf.ctypes.data, 1 << 17, C.byref(got), None) == L.E_INVALID
    assert lib.mpb_bgzf_compress_host(eng.ctx, None, 0, None, 0, C.byref(got), None) == 0 and got.value == 0
    assert lib.mpb_bgzf_compress_host(eng.ctx, b"abc", 3, buf.ctypes.data, 3 + 31, C.byref(got), None) == 0
    assert gzip.decompress(buf[:got.value].tobytes() + cli.BGZF_EOF) == b"abc"


def test_kernel_times_name_the_three_kernels(eng):
    eng.timing(True)
    eng.timing_reset()
    eng.bgzf_compress(B.golden_text())
    t = eng.kernel_times()
    eng.timing(False)
    assert all(t[k][1] == 1 and t[k][0] > 0 for k in ("bgzf_deflate", "bgzf_scan", "bgzf_frame")), t


@pytest.mark.parametrize("paired", [False, True], ids=["forward", "paired"])
def test_cli_golden_commands_with_device_compress(tmp_path, paired):
    from test_cli_golden import reference_args
    got, logs, calls = [], [], []
    for on in (False, True):
        out = str(tmp_path / ("on" if on else "off"))
        a = reference_args(paired=paired, forward_fastq=os.path.join(GOLD, "test1.fastq.gz"), output_prefix=out,
                           reverse_fastq=os.path.join(GOLD, "test2.fastq.bz2") if paired else None, output_compression="gz")
        a.device_compress = on
        be = cli.make_gpu_backend(None)
        log = io.StringIO()
        made = []
        inner = cli._DevicePaths.compress
        try:
            cli._DevicePaths.compress = lambda self, data: made.append(len(data)) or inner(self, data)
            assert cli.main(a, backend=be, out=log) == 0
        finally:
            cli._DevicePaths.compress = inner
            be.engine.close()
        calls.append(sum(made))
        logs.append(log.getvalue())
        files = sorted(p for p in os.listdir(str(tmp_path)) if p.startswith(os.path.basename(out) + "."))
        assert files and all(p.endswith(".gz") for p in files)
        texts = {}
        for p in files:
            blob = open(os.path.join(str(tmp_path), p), "rb").read()
            assert blob.endswith(cli.BGZF_EOF)
            texts[p.split(".", 1)[1]] = gzip.decompress(blob)
            assert read_back(blob)[0] == texts[p.split(".", 1)[1]]              # GzipReader, four threads
        got.append(texts)
    assert got[0].keys() == got[1].keys() and got[0] == got[1] and sum(len(v) for v in got[0].values()) > 100000
    assert calls[0] == 0 and calls[1] == sum(len(v) for v in got[1].values())   # every output byte went through the device
    assert not any("--device_compress" in l for l in logs)
