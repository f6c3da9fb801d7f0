"""The formatter kernels' lane code on the host (moira_amd/csrc/mpb_format_lane.inc through tests/helpers/format_lane_check.cpp,
built with -fsanitize=address,undefined together with csrc/fastio.cpp and run as a program; nothing is preloaded): 256 lane
states in lockstep, every load checked against the text's whole 16-byte words and the small arrays, every store against the
record's own output range and against a second store to the same byte.  The program compares with mio_format byte for byte over
the case list of tests/helpers/format_inputs.py; here the byte counts are checked again against fastio.format_records.  Two
sensitivity builds must fail named cases.  The kernels themselves: tests/test_gpu_format_text.py."""
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

from helpers import format_inputs as X
from moira_amd import fastio as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "moira_amd", "csrc")


def build(tmp, *defines):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = os.path.join(str(tmp), "check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "include"), "-I", CSRC] + list(defines) +
                          [os.path.join(ROOT, "tests", "helpers", "format_lane_check.cpp"), os.path.join(CSRC, "fastio.cpp"),
                           "-o", exe])
    return exe


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return build(tmp_path_factory.mktemp("format_model"))


def pack(c):
    kw = c["kw"]
    nsel = len(c["idx"]) if c["sel"] is None else len(c["sel"])
    relabel = kw.get("relabel")
    labels = [s.encode() for s in kw.get("labels") or []]
    off = kw.get("fastq_offset", 33)
    out_off = kw.get("out_offset")
    blob = [struct.pack("<32s3q10i", c["name"].encode(), len(c["idx"]), len(c["text"]), nsel, int(c["sel"] is not None), kw["kind"], off,
                        off if out_off is None else out_off, int(kw.get("clamp_q0", True)), kw.get("max_len", 0), int(relabel is not None),
                        len(relabel or ""), len(labels), int(kw.get("label_id") is not None)),
            c["idx"].tobytes(), c["text"]]
    if c["sel"] is not None:
        blob.append(c["sel"].tobytes())
    blob.append((relabel or "").encode())
    if relabel is not None:
        blob.append(np.ascontiguousarray(kw["relabel_index"], np.int64).tobytes())
    for s in labels:
        blob += [struct.pack("<i", len(s)), s]
    if kw.get("label_id") is not None:
        blob.append(np.ascontiguousarray(kw["label_id"], np.int32).tobytes())
    return b"".join(blob)


def run(exe, tmp, cases):
    fin = os.path.join(str(tmp), "cases.bin")
    with open(fin, "wb") as fh:
        fh.write(struct.pack("<i", len(cases)) + b"".join(pack(c) for c in cases))
    p = subprocess.run([exe, fin], capture_output=True, text=True)
    lines = {}
    for ln in p.stdout.splitlines():
        mt = re.match(r"case (\S+): (ok|refused|FAIL)(.*)", ln)
        if mt:
            lines[mt.group(1)] = (mt.group(2), mt.group(3).strip())
    return p.returncode, p.stdout[-3000:] + p.stderr[-3000:], lines


def check(exe, tmp, cases):
    rc, out, lines = run(exe, tmp, cases)
    assert rc == 0 and "%d cases, 0 loads out of bounds, 0 fail" % len(cases) in out, out
    assert set(lines) == {c["name"] for c in cases}
    return lines


def test_every_case_is_mio_formats_bytes(checker, tmp_path):
    cases = X.all_cases() + [X.fasta_ignores_quality_columns()]
    assert len({c["name"] for c in cases}) == len(cases)
    lines = check(checker, tmp_path, cases)
    for c in cases:
        assert lines[c["name"]] == ("ok", "bytes=%d" % len(X.want(c))), c["name"]


def test_records_of_65535_bases_are_mio_formats_bytes(checker, tmp_path):
    """Up to 512 steps of a lane group's running-base loop, every load and store checked (the kernels: tests/test_gpu_long_text.py)."""
    cases = X.long_cases()
    assert len({c["name"] for c in cases}) == len(cases)
    lines = check(checker, tmp_path, cases)
    for c in cases:
        assert lines[c["name"]] == ("ok", "bytes=%d" % len(X.want(c))), c["name"]


def test_the_equal_offset_form_keeps_a_byte_below_the_offset(checker, tmp_path):
    """put_qual_string copies the line when the offsets are equal and raises only the byte fastq_offset itself: q = -1 stays the
    byte it was there, while with different offsets it becomes the floor.  Both are mio_format's bytes."""
    text, idx = X.build([(b"r", b"ACGT", bytes([32, 33, 34, 32]))])
    same = X.case("below_same", text, idx, kind=F.FMT_FASTQ, fastq_offset=33, out_offset=33, clamp_q0=True)
    other = X.case("below_other", text, idx, kind=F.FMT_FASTQ, fastq_offset=33, out_offset=64, clamp_q0=True)
    check(checker, tmp_path, [same, other])
    assert X.want(same).endswith(b"+\n" + bytes([32, 34, 34, 32]) + b"\n")
    assert X.want(other).endswith(b"+\n" + bytes([65, 65, 65, 65]) + b"\n")


def test_damaged_rows_are_refused_without_a_load_out_of_bounds(checker, tmp_path):
    cases = X.damaged_cases()
    lines = check(checker, tmp_path, [c for c, _ in cases])
    for c, bad in cases:
        assert lines[c["name"]] == ("refused", "rowfail=%d" % bad), (c["name"], lines[c["name"]])


def test_an_upper_clamp_on_fastq_characters_fails_the_high_qualities(tmp_path):
    exe = build(tmp_path, "-DFM_WRONG_UPPER_CLAMP")
    cases = X.quality_cases() + X.max_len_cases()
    rc, out, lines = run(exe, tmp_path, cases)
    assert rc == 4, out
    for c in cases:
        high = c["name"].startswith("q_") and c["kw"]["kind"] == F.FMT_FASTQ
        assert lines[c["name"]][0] == ("FAIL" if high else "ok"), (c["name"], out)


def test_a_blank_behind_the_last_qual_value_fails_every_qual_record(tmp_path):
    exe = build(tmp_path, "-DFM_WRONG_TRAILING_BLANK")
    cases = X.max_len_cases() + X.length_cases()
    rc, out, lines = run(exe, tmp_path, cases)
    assert rc == 4, out
    for c in cases:
        assert lines[c["name"]][0] == ("FAIL" if c["kw"]["kind"] == F.FMT_QUAL else "ok"), (c["name"], out)
