"""CPU side of the device text pack (include/moira_pb.h: mpb_text_rows, mpb_pack_text_device, mpb_filter_text_host).

  * mpb_text_rows -- the only place the offsets of a text are trusted from -- against a numpy restatement, on an index
    that fastio's indexer built, and every refusal it owes;
  * the per-chunk code of k_pack_text, cut out of the kernel file and run on the host against mio_pack with checked loads
    (tests/helpers/pack_text_check.cpp);
  * the CLI switch --device_pack where it does not apply.
The kernel itself and the entries that need a device: tests/test_gpu_pack_text.py.
"""
import io
import os
import shutil
import subprocess

import numpy as np
import pytest

from moira_amd import _lib as L
from moira_amd import cli
from moira_amd import engine as E
from moira_amd import fastio as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def build_fastq(n=37, seed=5):
    """FASTQ text with LF and CRLF line ends whose final record has no newline -> (text, [(seq, qual)])."""
    rng = np.random.default_rng(seed)
    recs, parts = [], []
    for i in range(n):
        ln = int(rng.integers(1, 90))
        seq = "".join(rng.choice(list("ACGTNn"), ln, p=[.24, .24, .24, .24, .02, .02]))
        qual = "".join(chr(33 + int(v)) for v in rng.integers(0, 42, ln))
        recs.append((seq, qual))
        nl = "\r\n" if i % 3 == 1 else "\n"
        last = i == n - 1
        parts.append("@r%d some text%s%s%s+%s%s%s" % (i, nl, seq, nl, nl, qual, "" if last else nl))
    return "".join(parts).encode(), recs


@pytest.fixture(scope="module")
def indexed():
    text, recs = build_fastq()
    idx, consumed, err = F.index(text, True, 1000)
    assert err is None and len(idx) == len(recs) and consumed == len(text)
    assert idx[-1, F.QUAL_OFF] + idx[-1, F.QUAL_LEN] == len(text)           # the last record ends at the last byte
    return text, recs, idx


def model_rows(idx, sel, max_len):
    """numpy restatement of the descriptors: record sel[k]'s two offsets and min(QUAL_LEN, max_len)."""
    r = idx if sel is None else idx[np.asarray(sel, np.int64)]
    ln = r[:, F.QUAL_LEN].copy()
    if max_len > 0:
        ln = np.minimum(ln, max_len)
    return r[:, F.SEQ_OFF], r[:, F.QUAL_OFF], ln


def test_header_restates_the_index_columns():
    """moira_pb.h restates moira_io.h's column numbers (the two libraries do not include each other)."""
    import re
    pb = open(os.path.join(ROOT, "include", "moira_pb.h")).read()
    io_h = open(os.path.join(ROOT, "include", "moira_io.h")).read()
    for a, b in (("MPB_IDX_SEQ_OFF", "MIO_SEQ_OFF"), ("MPB_IDX_QUAL_OFF", "MIO_QUAL_OFF"), ("MPB_IDX_QUAL_LEN", "MIO_QUAL_LEN"),
                 ("MPB_IDX_COLS", "MIO_IDX_COLS")):
        va = int(re.search(r"#define %s\s+(\d+)" % a, pb).group(1))
        vb = int(re.search(r"#define %s\s+(\d+)" % b, io_h).group(1))
        assert va == vb, (a, b)
    assert (F.SEQ_OFF, F.QUAL_OFF, F.QUAL_LEN, F.IDX_COLS) == (2, 4, 5, 6)
    assert E.TEXT_ROW_DTYPE.itemsize == 24 and C_sizeof_row() == 24
    assert L.K_PACK_TEXT == 11 and L.KERNEL_NAMES[11] == "pack_text" and len(L.KERNEL_NAMES) == 12


def C_sizeof_row():
    import ctypes
    return ctypes.sizeof(L.TextRow)


@pytest.mark.parametrize("sel_kind", ["none", "permuted", "repeats"])
@pytest.mark.parametrize("max_len", [0, 1, 16, 40, 89, 500])
def test_text_rows_equal_the_numpy_restatement(indexed, sel_kind, max_len):
    text, recs, idx = indexed
    n = len(idx)
    rng = np.random.default_rng(11)
    sel = {"none": None, "permuted": rng.permutation(n), "repeats": rng.integers(0, n, 2 * n + 3)}[sel_kind]
    so, qo, ln = model_rows(idx, sel, max_len)
    # the sequence and quality bytes the descriptors point at are the records' own
    for k in (0, len(ln) // 2, len(ln) - 1):
        r = k if sel is None else int(sel[k])
        assert text[so[k]:so[k] + ln[k]].decode() == recs[r][0][:ln[k]] and text[qo[k]:qo[k] + ln[k]].decode() == recs[r][1][:ln[k]]
    rows, longest = E.text_rows(idx, sel, text_bytes=len(text), max_len=max_len, stride=0)
    assert rows is None and longest == int(ln.max())                         # stride 0: the longest packed length only
    stride = (longest + 127) // 128 * 128
    rows, longest2 = E.Engine.text_rows(idx, sel, text_bytes=len(text), max_len=max_len, stride=stride)
    assert longest2 == longest and len(rows) == len(ln)
    assert np.array_equal(rows["seq_off"], so) and np.array_equal(rows["qual_off"], qo)
    assert np.array_equal(rows["len"], ln) and not rows["pad"].any()


def test_truncation_below_equal_and_above_one_read(indexed):
    text, recs, idx = indexed
    k = int(np.argmax(idx[:, F.QUAL_LEN]))
    full = int(idx[k, F.QUAL_LEN])
    for max_len, want in ((full - 1, full - 1), (full, full), (full + 1, full)):
        rows, longest = E.text_rows(idx, [k], text_bytes=len(text), max_len=max_len, stride=128)
        assert rows["len"].tolist() == [want] and longest == want


def refused(idx, sel, text_bytes, max_len=0, stride=128, n_records=None):
    with pytest.raises(ValueError) as e:
        E.text_rows(idx if n_records is None else idx[:n_records], sel, text_bytes=text_bytes, max_len=max_len, stride=stride)
    return e.value.bad_record


def test_every_refusal_names_the_record(indexed):
    text, recs, idx = indexed
    n, tb = len(idx), len(text)
    # a record that ends exactly at text_bytes is accepted; one byte less of text refuses it (the last record, position n - 1)
    E.text_rows(idx, None, text_bytes=tb, stride=128)
    assert refused(idx, None, tb - 1) == n - 1
    sel = [5, n - 1, 3]
    assert refused(idx, sel, tb - 1) == 1                                   # ... reported by its position in sel order
    # the sequence line one byte past the text
    bad = idx.copy()
    bad[7, F.SEQ_OFF] = tb - bad[7, F.QUAL_LEN] + 1
    assert refused(bad, None, tb) == 7
    bad[7, F.SEQ_OFF] = tb - bad[7, F.QUAL_LEN]
    E.text_rows(bad, None, text_bytes=tb, stride=128)
    # negative offsets
    for col in (F.SEQ_OFF, F.QUAL_OFF):
        bad = idx.copy()
        bad[4, col] = -1
        assert refused(bad, None, tb) == 4
        assert refused(bad, [9, 9, 4], tb) == 2
    # sel outside the index, above and below
    assert refused(idx, [0, n], tb) == 1
    assert refused(idx, [-1], tb) == 0
    assert refused(idx, [0, 1, n - 1], tb, n_records=n - 1) == 2
    # a length of 65536 (in a text that could hold it), and 65535 is fine
    bad = idx.copy()
    bad[2, F.SEQ_OFF] = bad[2, F.QUAL_OFF] = 0
    bad[2, F.QUAL_LEN] = 65536
    assert refused(bad, None, 1 << 20, stride=0) == 2
    bad[2, F.QUAL_LEN] = 65535
    assert E.text_rows(bad, None, text_bytes=1 << 20, stride=0)[1] == 65535
    # a length of row_stride + 1
    longest = int(idx[:, F.QUAL_LEN].max())
    k = int(np.argmax(idx[:, F.QUAL_LEN]))
    assert refused(idx, None, tb, stride=longest - 1) == k
    E.text_rows(idx, None, text_bytes=tb, stride=longest)
    E.text_rows(idx, None, text_bytes=tb, max_len=longest - 1, stride=longest - 1)      # truncation brings it inside
    # nothing to do
    rows, longest0 = E.text_rows(idx, [], text_bytes=tb, stride=128)
    assert len(rows) == 0 and longest0 == 0
    lib = L.load()
    assert lib.mpb_text_rows(None, 0, None, 0, 0, 0, 0, None, None, None) == 0


def test_pack_text_chunk_code_equals_mio_pack_on_the_host(tmp_path):
    """k_pack_text's per-chunk code (the aligned fetch, the byte-align funnel, the four-bases-at-a-time rules) is plain integer
    code: it is cut out of the kernel file and run on the host, every row chunk by chunk as the lanes do, against mio_pack --
    matrix, lengths, flags, first bad record and message kind -- with every 16-byte load checked against
    [text, text + round_up(text_bytes, 16)) and the bytes past text_bytes filled with 0xFF and with 'N' in turn."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    src = open(os.path.join(ROOT, "moira_amd", "csrc", "mpb_kernels.hip")).read()
    # the decoders' rules (decode4_bytes .. decode16: from one function's signature to the next one's) and the chunk code between
    # its two marks
    a = src.index("__device__ __forceinline__ uint32_t decode4_bytes(")
    b = src.index("__device__ __forceinline__ uint32_t lower_as_q254(")
    c = src.index("// [k_pack_text chunk code: begin]")
    d = src.index("// [k_pack_text chunk code: end]")
    (tmp_path / "pack_text_funcs.h").write_text(src[a:b] + src[c:d])
    exe = str(tmp_path / "check")
    csrc = os.path.join(ROOT, "moira_amd", "csrc")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-I", str(tmp_path), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "helpers", "pack_text_check.cpp"), os.path.join(csrc, "fastio.cpp"),
                           os.path.join(csrc, "inflate.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "0 loads out of bounds, 0 mismatches" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


# ---- the CLI switch -----------------------------------------------------------------------------------------------------

def test_device_pack_parses_and_is_off_by_default():
    base = ["-ffq", "a.fastq", "-c", "false", "-me", "3", "-n", "disallow", "-t", "200"]
    off, on = cli.parse_arguments(base), cli.parse_arguments(base + ["--device_pack"])
    assert off.device_pack is False and on.device_pack is True
    d_off, d_on = dict(vars(off)), dict(vars(on))
    d_off.pop("device_pack"), d_on.pop("device_pack")
    assert d_off == d_on                                                    # nothing else moves
    assert d_off["collapse"] is False and d_off["maxerrors"] == 3 and d_off["truncate"] == 200 and d_off["fast_discard"] is False
    assert "--device_pack" in cli.build_parser().format_help()


def test_device_pack_on_a_cpu_backend_says_so_once_and_changes_nothing(tmp_path, oracle):
    from test_cli_golden import oracle_backend, reference_args
    outs, said = [], []
    for name, on in (("off", False), ("on", True)):
        out = str(tmp_path / name)
        msg = io.StringIO()
        a = reference_args(paired=False, forward_fastq=os.path.join(GOLD, "test1.fastq.gz"), output_prefix=out, collapse=False)
        if on:
            a.device_pack = True
        assert cli.main(a, backend=oracle_backend(oracle), out=msg) == 0
        said.append([l for l in msg.getvalue().split("\n") if "device_pack" in l])
        outs.append({k: open("%s.qc.%s" % (out, k), "rb").read() for k in ("good.fasta", "good.qual", "bad.fasta", "bad.qual")})
    assert said[0] == [] and len(said[1]) == 1 and "host packing is used" in said[1][0]
    assert outs[0] == outs[1] and len(outs[0]["good.fasta"]) > 0
