"""The collapse kernels' lane code on the host (moira_amd/csrc/mpb_collapse_lane.inc through tests/helpers/collapse_lane_check.cpp,
built with -fsanitize=address,undefined together with csrc/fastio.cpp and run as a program; nothing is preloaded): one lane per
record, 256 lane states in lockstep, every load checked against the text's whole 16-byte words and the small arrays, every store
and modelled atomic against its array.  Each case of tests/helpers/collapse_inputs.py runs with the records handed to the lanes
in order and in a seeded shuffled order; hash must be mio_py2_hash's, rep the first record with the same truncated bytes, both
equal between the two runs; here the group counts are checked again against the Python oracle.
THE BYTE COMPARE IS PINNED HERE.  k_col_group reads hash[] as an input, and a real collision of two 64-bit hashes cannot be
constructed for a GPU test; so the program also runs cases with forged hashes -- one value for every record, and values that
differ but start every probe walk at one slot -- and rep must still be the oracle's.  Two sensitivity builds must fail named
cases.  The kernels themselves: tests/test_gpu_collapse_text.py."""
import os
import re
import shutil
import struct
import subprocess

import pytest

from helpers import collapse_inputs as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "moira_amd", "csrc")


def build(tmp, *defines):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = os.path.join(str(tmp), "check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "include"), "-I", CSRC] + list(defines) +
                          [os.path.join(ROOT, "tests", "helpers", "collapse_lane_check.cpp"), os.path.join(CSRC, "fastio.cpp"),
                           "-o", exe])
    return exe


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return build(tmp_path_factory.mktemp("collapse_model"))


def pack(c):
    return struct.pack("<32s2q2i", c["name"].encode(), len(c["idx"]), len(c["text"]), c["max_len"], c["forge"]) + c["idx"].tobytes() + c["text"]


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


def groups(c):
    return len(set(X.sequences(c)))


def test_every_case_is_the_oracles_hash_and_first_equal_record(checker, tmp_path):
    cases = X.all_cases()
    assert len({c["name"] for c in cases}) == len(cases)
    lines = check(checker, tmp_path, cases)
    for c in cases:
        assert lines[c["name"]] == ("ok", "n=%d groups=%d" % (len(c["idx"]), groups(c))), c["name"]


def test_sequences_of_65535_bases_are_the_oracles(checker, tmp_path):
    """cl_hash and cl_equal over 4,096 words a sequence, every load checked (the kernels: tests/test_gpu_long_text.py)."""
    cases = X.long_cases()
    lines = check(checker, tmp_path, cases)
    for c in cases:
        assert lines[c["name"]] == ("ok", "n=%d groups=%d" % (len(c["idx"]), groups(c))), c["name"]
    assert [groups(c) for c in cases] == [8, 3]


def test_forged_hashes_leave_rep_to_the_byte_compare(checker, tmp_path):
    cases = X.forged_cases()
    lines = check(checker, tmp_path, cases)
    for c in cases:
        assert lines[c["name"]] == ("ok", "n=%d groups=%d" % (len(c["idx"]), groups(c))), c["name"]


def test_bad_rows_are_refused_without_a_load_out_of_bounds(checker, tmp_path):
    cases = X.bad_row_cases()
    lines = check(checker, tmp_path, [c for c, _ in cases])
    for c, bad in cases:
        assert lines[c["name"]] == ("refused", "rowfail=%d" % bad), (c["name"], lines[c["name"]])


def test_without_the_byte_compare_the_forged_hash_cases_fail(tmp_path):
    exe = build(tmp_path, "-DCL_SKIP_BYTE_COMPARE")
    cases = X.forged_cases() + X.small_cases() + X.truncation_cases()
    rc, out, lines = run(exe, tmp_path, cases)
    assert rc == 4, out
    for c in cases:
        assert lines[c["name"]][0] == ("FAIL" if c["forge"] == 1 else "ok"), (c["name"], out)


def test_without_the_max_len_clamp_the_truncation_case_fails(tmp_path):
    exe = build(tmp_path, "-DCL_NO_MAX_LEN_CLAMP")
    cases = X.truncation_cases() + X.small_cases()
    rc, out, lines = run(exe, tmp_path, cases)
    assert rc == 4, out
    for c in cases:
        assert lines[c["name"]][0] == ("FAIL" if c["name"] == "truncation_on" else "ok"), (c["name"], out)
