"""The lane code of mpb_format_records_host on the host (moira_amd/csrc/mpb_format_lane.inc with the report kind, the ee suffix
and aux, through tests/helpers/format_records_check.cpp, built with -fsanitize=address,undefined together with csrc/fastio.cpp
and run as a program; nothing is preloaded): 256 lane states in lockstep, every load checked against its array, every store
against the record's own output range and against a second store to the same byte.  The program compares with mio_format(ee) /
mio_format_report byte for byte over the case list of tests/helpers/format_records_inputs.py; here the byte counts are checked
again against fastio.format_records / fastio.format_report.  Two sensitivity builds must fail exactly the cases they name.  The
kernels themselves: tests/test_gpu_format_records.py."""
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

from helpers import format_records_inputs as R
from moira_amd import fastio as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "moira_amd", "csrc")


def build(tmp, *defines):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = os.path.join(str(tmp), "check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "include"), "-I", CSRC] + list(defines) +
                          [os.path.join(ROOT, "tests", "helpers", "format_records_check.cpp"), os.path.join(CSRC, "fastio.cpp"),
                           "-o", exe])
    return exe


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return build(tmp_path_factory.mktemp("format_records_model"))


def pack(c):
    kw = c["kw"]
    nsel = len(c["idx"]) if c["sel"] is None else len(c["sel"])
    relabel = kw.get("relabel")
    labels = [s.encode() for s in kw.get("labels") or []]
    off = kw.get("fastq_offset", 33)
    out_off = kw.get("out_offset")
    ee, aux = kw.get("ee"), kw.get("aux")
    blob = [struct.pack("<32s3q12i", c["name"].encode(), len(c["idx"]), len(c["text"]), nsel, int(c["sel"] is not None), kw["kind"], off,
                        off if out_off is None else out_off, int(kw.get("clamp_q0", True)), kw.get("max_len", 0), int(relabel is not None),
                        len(relabel or ""), len(labels), int(kw.get("label_id") is not None), int(ee is not None), int(aux is not None)),
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
    if ee is not None:
        assert len(ee) == nsel
        blob.append(np.ascontiguousarray(ee, np.float64).tobytes())
    if aux is not None:
        assert np.shape(aux) == (len(c["idx"]), 3)
        blob.append(np.ascontiguousarray(aux, np.int32).tobytes())
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


def test_every_case_is_the_host_formatters_bytes(checker, tmp_path):
    cases = R.all_cases()
    assert len({c["name"] for c in cases}) == len(cases) and all(len(c["name"]) < 32 for c in cases)
    lines = check(checker, tmp_path, cases)
    for c in cases:
        assert lines[c["name"]] == ("ok", "bytes=%d" % len(R.want(c))), c["name"]


def test_the_case_list_holds_what_it_says():
    aux = R.base_aux()
    for col in range(3):
        assert set(aux[:, col].tolist()) == set(R.AUX_VALUES)
    text, idx = R.base_text()
    assert set(idx[:, 1].tolist()) == {1, 15, 16, 17, 300} and len(idx) == len(aux)
    assert any(R.rounds_down_on_a_tie(v) for v in R.EE) and not R.rounds_down_on_a_tie(0.375) and R.rounds_down_on_a_tie(0.125)
    # the suffix as glibc prints it, for the values that are easy to get wrong
    got = bytes(F.format_records(*R.X.build([(b"r", b"A", b"I")] * 6), np.arange(6), F.FMT_FASTA,
                                 ee=np.array([-0.0, -0.001, 0.125, 0.375, 0.005, float(2 ** 53 - 1)])))
    assert [ln.split(b";")[1] for ln in got.split(b"\n")[0::2][:6]] == [b"ee=-0.00", b"ee=-0.00", b"ee=0.12", b"ee=0.38", b"ee=0.01",
                                                                        b"ee=9007199254740991.00"]


def test_what_lies_outside_is_refused_at_its_record_without_a_load_out_of_bounds(checker, tmp_path):
    cases = R.refused_cases()
    lines = check(checker, tmp_path, [c for c, _ in cases])
    for c, bad in cases:
        assert lines[c["name"]] == ("refused", "rowfail=%d" % bad), (c["name"], lines[c["name"]])


def test_rounding_ties_half_up_fails_the_ties_that_round_down(tmp_path):
    exe = build(tmp_path, "-DFM_WRONG_TIES_HALF_UP")
    cases = R.tie_cases() + R.sign_cases()
    rc, out, lines = run(exe, tmp_path, cases)
    assert rc == 4, out
    for c in cases:
        ee = c["kw"].get("ee")
        tie = ee is not None and any(R.rounds_down_on_a_tie(v) for v in ee)
        assert tie == c["name"].startswith(("ties_", "aux_negative_ee", "aux_none_fastq")), c["name"]
        assert lines[c["name"]][0] == ("FAIL" if tie else "ok"), (c["name"], out)


def test_dropping_the_minus_sign_fails_the_negative_aux_values(tmp_path):
    exe = build(tmp_path, "-DFM_WRONG_AUX_SIGN")
    cases = R.sign_cases() + R.tie_cases()
    rc, out, lines = run(exe, tmp_path, cases)
    assert rc == 4, out
    for c in cases:
        neg = c["kw"]["kind"] == R.REPORT and bool((np.asarray(c["kw"]["aux"]) < 0).any())
        assert neg == c["name"].startswith("aux_negative"), c["name"]
        assert lines[c["name"]][0] == ("FAIL" if neg else "ok"), (c["name"], out)
