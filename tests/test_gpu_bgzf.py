"""k_bgzf_deflate, k_bgzf_scan and k_bgzf_frame on the GPU (include/moira_pb.h: mpb_bgzf_compress_host; Engine.bgzf_compress; the
CLI's --device_compress).  Every input goes through the same checks: gzip reads the output back, each member's BSIZE, CRC and
ISIZE are right and its deflate stream inflates ON ITS OWN (a member is its own window), the package's reader gives the text
back on several threads, the output fits mpb_bgzf_bound, and a second call gives the same bytes.  And every member's stream is,
byte for byte, the one the host lane model writes for its text in the kernel's documented order (all look-ups of a step, then
its insertions with the largest position winning): length, SHA-256, block type and the call's counts against
tests/golden/bgzf_model_streams.json, which tests/test_bgzf_model_streams.py holds to the model.  The lane code on the CPU:
tests/test_bgzf_lane_model.py; the writer and the switch: tests/test_bgzf_writer.py."""
import ctypes as C
import gzip
import hashlib
import io
import os
import zlib

import numpy as np
import pytest

from helpers import bgzf_inputs as B
from helpers import bgzf_model as M
from moira_amd import _lib as L
from moira_amd import cli
from moira_amd import engine as E
from moira_amd import fastio as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
NAMED = dict(B.named_inputs())
FIXTURE = M.load()


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


def stream_btype(stream):
    """BTYPE of a member's one block: the stream's first three bits are BFINAL = 1 and BTYPE (a stored block's first byte is 1)."""
    assert stream[0] & 1
    return M.STORED if stream[0] == 1 else (stream[0] >> 1) & 3


def model_sums(entries):
    """what bgzf_stats() gives for a call over these members of the fixture, but `members`"""
    sums = {"dynamic": sum(e["btype"] == M.DYNAMIC for e in entries), "fixed": sum(e["btype"] == M.FIXED for e in entries),
            "stored": sum(e["btype"] == M.STORED for e in entries)}
    for stat, key in (("literals", "literals"), ("matches", "matches"), ("matched_bytes", "matched")):
        sums[stat] = sum(e[key] for e in entries)
    return sums


def equal_the_model(what, ms, entries, st):
    """The members of the device's output (B.split_bgzf's rows) against the fixture's entries for the same texts, byte for byte:
    every stream's length, SHA-256 and block type, and the call's counts against the sums of the model's."""
    assert len(ms) == len(entries), (what, len(ms), len(entries))
    sums = model_sums(entries)
    counts = "the call's counts: device %s, model %s" % ({k: st[k] for k in sums}, sums)
    for k, ((_, stream, _, isize), e) in enumerate(zip(ms, entries)):
        btype = stream_btype(stream)
        same = len(stream) == e["bytes"] and btype == e["btype"] and isize == e["n"] and hashlib.sha256(stream).hexdigest() == e["sha256"]
        assert same, ("%s, member %d of %d (%d bytes of text): the device's stream has %d bytes and block type %d, the model's %d and %d; %s"
                      % (what, k, len(ms), e["n"], len(stream), btype, e["bytes"], e["btype"], counts))
    assert {k: st[k] for k in sums} == sums, "%s: %s" % (what, counts)


def compress_checked(eng, text, name):
    """Engine.bgzf_compress(text) with every check of the module's docstring -> (output, stats).  `name`: the input's name in
    the fixture of the host lane model's streams; an input without an entry is an error."""
    entries = FIXTURE[name]
    assert [e["n"] for e in entries] == [len(m) for m in B.members(text)], name
    out = eng.bgzf_compress(text)
    st = dict(eng.bgzf_stats())
    equal_the_model(name, B.split_bgzf(out), entries, st)
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
    out, st = compress_checked(eng, text, name)
    assert st["members"] == -(-len(text) // B.DATA)
    if not text:
        assert out == b"" and st == dict.fromkeys(st, 0)


def test_one_byte_over_a_whole_member(eng):
    out, st = compress_checked(eng, NAMED["one_byte_member"], "one_byte_member")
    assert st["literals"] == 1 and st["matches"] == -(-(B.DATA - 1) // 258) and len(out) < 400      # distance 1, the cap of 258


@pytest.mark.parametrize("period", [3, 64, B.STEP - 1, B.STEP + 1])
def test_periods_around_the_step(eng, period):
    text = NAMED["period%d" % period]
    out, st = compress_checked(eng, text, "period%d" % period)
    assert st["matched_bytes"] >= len(text) - 3 * max(period, B.STEP)


def test_the_largest_legal_distance_and_the_first_illegal_one(eng):
    _, st = compress_checked(eng, NAMED["period32768"], "period32768")
    assert st["matched_bytes"] >= (B.DATA - 32768) // 2
    _, st = compress_checked(eng, NAMED["period32769"], "period32769")
    assert st["matched_bytes"] < 3000


def test_a_repeat_across_the_member_border_is_not_matched(eng):
    text = NAMED["repeat_across_border"]
    out, st = compress_checked(eng, text, "repeat_across_border")   # (every member inflates on its own there)
    assert st["members"] == 2 and st["matched_bytes"] < 300


def test_random_bytes_come_out_stored_or_fixed(eng):
    out, st = compress_checked(eng, NAMED["random_member"], "random_member")
    assert (st["members"], st["stored"]) == (1, 1) and len(out) == B.DATA + 31
    out, st = compress_checked(eng, NAMED["random_1000"], "random_1000")
    assert st["dynamic"] == 0 and len(out) <= 1000 + 31


def test_all_byte_values_twice_and_a_text_without_a_repeat(eng):
    _, st = compress_checked(eng, NAMED["all_bytes_twice"], "all_bytes_twice")
    assert st["matched_bytes"] >= 250
    out, st = compress_checked(eng, NAMED["no_repeat"], "no_repeat")
    assert st["matches"] == 0 and st["dynamic"] == 1 and len(out) < len(NAMED["no_repeat"])        # zero distance codes
    _, st = compress_checked(eng, NAMED["min_match_at_end"], "min_match_at_end")                    # exactly one distance code
    assert (st["matches"], st["matched_bytes"], st["literals"]) == (1, 3, 703)


@pytest.mark.parametrize("which", [0, 1, 2], ids=["fastq", "fasta", "qual"])
def test_golden_texts(eng, which):
    text = B.golden_renderings()[which]
    out, st = compress_checked(eng, text, M.GOLDEN_NAMES[which])
    assert st["stored"] == 0 and len(out) < len(text)


def test_fuzz_members(eng):
    for k in range(20):
        compress_checked(eng, B.fuzz_member(k), "fuzz%d" % k)


@pytest.mark.parametrize("name", [n for n, _ in B.model_inputs()])
def test_model_inputs_equal_the_model(eng, name):
    """The members at which the workgroup's own parts can leave the model: the last words of the bit buffer, codes of 15 bits,
    both limits of the length builder, hundreds of positions of a step in one bucket, a match of 258 as the last token."""
    text = dict(B.model_inputs())[name]
    _, st = compress_checked(eng, text, name)
    assert st["members"] == 1


def test_more_members_than_compute_units(eng):
    """300 members in one call: a workgroup holds a CU's LDS alone, so workgroups follow each other on a CU, each with the LDS
    the one before it left.  Every member equals the model for its text wherever it lies in the grid."""
    both = dict(B.named_inputs() + B.model_inputs())
    names = ["len%d" % B.DATA, "buffer_nearly_full", "random_member", "period5_member", "period32768", "one_byte_member"]
    assert all(len(both[n]) == B.DATA for n in names) and len({both[n] for n in names}) == 6
    order = [names[k % 6] for k in range(300)]
    text = b"".join(both[n] for n in order)
    out = eng.bgzf_compress(text)
    st = dict(eng.bgzf_stats())
    assert st["members"] == 300
    ms = B.split_bgzf(out)                                          # (asserts that the framed output is dense)
    equal_the_model("300 members", ms, [FIXTURE[n][0] for n in order], st)
    assert all(crc == zlib.crc32(both[n]) and bsize == len(stream) + 25 for (bsize, stream, crc, _), n in zip(ms, order))
    assert eng.bgzf_compress(text) == out and eng.bgzf_stats() == st


def test_a_call_across_the_default_piece_size(eng, monkeypatch):
    """1,025 members with no piece size set: the default piece of 1,024 members (k_bgzf_scan with all its 1,024 entries), then a
    piece of one short member."""
    monkeypatch.delenv("MPB_BGZF_PIECE_MEMBERS", raising=False)
    name, last = "len%d" % B.DATA, "len257"
    text = NAMED[name] * 1024 + NAMED[last]
    out = eng.bgzf_compress(text)
    st = dict(eng.bgzf_stats())
    assert st["members"] == 1025
    entries = [FIXTURE[name][0]] * 1024 + [FIXTURE[last][0]]
    assert len(out) == sum(e["bytes"] + 26 for e in entries)
    equal_the_model("1025 members", B.split_bgzf(out), entries, st)


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
