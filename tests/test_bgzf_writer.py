"""The CPU half of --device_compress: _BlockCompressedWriter with a compressor handed in (batching, order, the carry, close()
with a partial batch, the end marker, the fallback when the compressor raises), the switch where it does not apply, and
mpb_bgzf_bound against its formula.  The kernels: tests/test_gpu_bgzf.py; their lane code: tests/test_bgzf_lane_model.py."""
import ctypes as C
import gzip
import io
import os

import numpy as np
import pytest

from moira_amd import _lib as L
from moira_amd import cli

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
W = cli._BlockCompressedWriter


class FakeCompressor:
    """compress() is the host's bgzf_compress at level 1 (so that its members can be told from the fallback's), and remembers
    what it was given; `refuse`: the texts (by their first 64 bytes) whose call raises.  The writer calls it from pool threads:
    the calls of different batches may arrive in any order, only the file is in order."""

    def __init__(self, refuse=()):
        import threading
        self.seen, self.reports, self.refuse, self.lock = [], [], set(refuse), threading.Lock()

    def compress(self, data):
        data = bytes(data)
        with self.lock:
            self.seen.append(data)
        if data[:64] in self.refuse:
            raise RuntimeError("HIP error: planted")
        return cli.bgzf_compress(data, 1)

    def report(self, e):
        with self.lock:
            self.reports.append(str(e))


def batches_of(text):
    step = W.BATCH_BLOCKS * W.BLOCK
    return [text[k:k + step] for k in range(0, len(text), step)]


def text_of(n, seed=0):
    return np.random.default_rng(seed).integers(65, 75, n).astype(np.uint8).tobytes()


def write_in_pieces(w, text, piece):
    for k in range(0, len(text), piece):
        assert w.write(text[k:k + piece]) == len(text[k:k + piece])


@pytest.mark.parametrize("piece", [1 << 22, 700001, 4097])
def test_batches_are_whole_blocks_in_order_and_close_sends_the_partial_one(tmp_path, piece):
    text = text_of(W.BATCH_BLOCKS * W.BLOCK * 2 + 3 * W.BLOCK + 12345, 1)
    fc = FakeCompressor()
    path = str(tmp_path / "o.gz")
    w = W(path, "gz", fc)
    write_in_pieces(w, text, piece)
    w.close()
    want = batches_of(text)                                                     # two full batches, then the partial one with the carry
    assert [len(b) for b in want] == [W.BATCH_BLOCKS * W.BLOCK] * 2 + [3 * W.BLOCK + 12345]
    assert sorted(fc.seen) == sorted(want)                                      # every batch once, whole blocks
    blob = open(path, "rb").read()
    assert blob.endswith(cli.BGZF_EOF) and blob == b"".join(cli.bgzf_compress(b, 1) for b in want) + cli.BGZF_EOF     # in order
    assert gzip.decompress(blob) == text and not fc.reports


def test_an_empty_output_is_the_end_marker_alone(tmp_path):
    fc = FakeCompressor()
    w = W(str(tmp_path / "e.gz"), "gz", fc)
    w.close()
    assert open(str(tmp_path / "e.gz"), "rb").read() == cli.BGZF_EOF and not fc.seen


def test_a_batch_the_compressor_refuses_goes_through_the_host_and_is_reported(tmp_path):
    text = text_of(W.BATCH_BLOCKS * W.BLOCK * 3 + 777, 2)
    bt = batches_of(text)
    fc = FakeCompressor(refuse=(bt[1][:64], bt[3][:64]))
    path = str(tmp_path / "f.gz")
    w = W(path, "gz", fc)
    write_in_pieces(w, text, 1 << 21)
    w.close()
    assert len(fc.seen) == 4 and len(fc.reports) == 2 and "planted" in fc.reports[0]
    blob = open(path, "rb").read()
    assert gzip.decompress(blob) == text
    # the refused batches are the host's own members, block by block (level 4), between the compressor's
    want = [cli.bgzf_compress(bt[0], 1), b"".join(cli.bgzf_compress(bt[1][k:k + W.BLOCK], 4) for k in range(0, len(bt[1]), W.BLOCK)),
            cli.bgzf_compress(bt[2], 1), cli.bgzf_compress(bt[3], 4), cli.BGZF_EOF]
    assert blob == b"".join(want)


def test_without_a_compressor_and_for_bz2_the_writer_is_unchanged(tmp_path):
    import bz2
    text = text_of(3 * W.BLOCK + 5, 3)
    w = W(str(tmp_path / "h.gz"), "gz")
    w.write(text); w.close()
    blob = open(str(tmp_path / "h.gz"), "rb").read()
    assert blob == b"".join(cli.bgzf_compress(text[k:k + W.BLOCK], 4) for k in range(0, len(text), W.BLOCK)) + cli.BGZF_EOF
    fc = FakeCompressor()
    w = W(str(tmp_path / "h.bz2"), "bz2", fc)                                   # a .bz2 output never uses it
    w.write(text); w.close()
    assert bz2.decompress(open(str(tmp_path / "h.bz2"), "rb").read()) == text and not fc.seen


def run_cli(tmp_path, name, oracle, **kw):
    from test_cli_golden import oracle_backend, reference_args
    out = str(tmp_path / name)
    a = reference_args(paired=False, forward_fastq=os.path.join(GOLD, "test1.fastq.gz"), output_prefix=out, silent=True, **kw)
    log = io.StringIO()
    assert cli.main(a, backend=oracle_backend(oracle), out=log) == 0
    files = sorted(p for p in os.listdir(str(tmp_path)) if p.startswith(name + "."))
    return {p.split(".", 1)[1]: open(os.path.join(str(tmp_path), p), "rb").read() for p in files}, log.getvalue()


@pytest.mark.parametrize("oc", ["none", "gz"])
def test_the_switch_where_it_does_not_apply_says_so_once_and_changes_no_file(tmp_path, oracle, oc):
    """A backend without a device engine (and, for `none`, no -oc gz): one line, the same files."""
    off, log_off = run_cli(tmp_path, "off", oracle, output_compression=oc)
    on, log_on = run_cli(tmp_path, "on", oracle, output_compression=oc, device_compress=True)
    assert "--device_compress" not in log_off
    assert log_on.count("--device_compress does not apply to this run") == 1 and "host zlib is used" in log_on
    assert off.keys() == on.keys() and len(off) >= 6 and off == on
    quiet, log_quiet = run_cli(tmp_path, "quiet", oracle, output_compression=oc, device_compress=True, nowarnings=True)
    assert "--device_compress" not in log_quiet and quiet == off


def test_the_parser_knows_the_switch_and_it_is_off_by_default():
    p = cli.build_parser()
    assert p.parse_args(["-ffq", "x"]).device_compress is False
    assert p.parse_args(["-ffq", "x", "--device_compress"]).device_compress is True
    assert "--device_compress" in p.format_help()


def test_bound_is_its_formula():
    lib = L.load()
    cap = C.c_int64(-1)
    for n in (0, 1, 0xff00, 0xff00 + 1, 5 * 0xff00, 5 * 0xff00 + 1, 1 << 40):
        assert lib.mpb_bgzf_bound(n, C.byref(cap)) == 0
        assert cap.value == n + 31 * -(-n // 0xff00), n
    assert [lib.mpb_bgzf_bound(n, C.byref(cap)) or cap.value for n in (0, 1, 0xff00, 0xff00 + 1)] == [0, 32, 0xff00 + 31, 0xff00 + 1 + 62]
    assert lib.mpb_bgzf_bound(-1, C.byref(cap)) == L.E_INVALID and b"mpb_bgzf_bound" in lib.mpb_last_error()
    assert lib.mpb_bgzf_bound(5, None) == L.E_INVALID
    assert L.BGZF_DATA == 0xff00 == cli.BGZF_DATA
