"""The fasta+qual record stage's lane code on the host (moira_amd/csrc/mpb_fasta_qual_lane.inc through
tests/helpers/fasta_qual_lane_check.cpp, built with -fsanitize=address,undefined together with csrc/fastio.cpp and run as a
program; nothing is preloaded): the line kernels over both texts, then 256 lane states in lockstep, every load checked against
the texts' whole 16-byte words and the line tables, every store against the record's own slot and against a second store to the
same byte.  The program compares every case it takes with mio_fasta_qual_index itself -- n, both consumed, out_used, out, the
rows -- and fails when it takes texts the host calls unsupported; here the hand-backs' reasons are checked, and the taken
cases once more against fastio.fasta_qual_index.  Two sensitivity builds must fail named cases.  The kernels themselves:
tests/test_gpu_fasta_qual.py.

"007" is three digits of value 7 and is taken, as the host takes it; "0007" is handed back (TOKEN), which the host would read:
the superset the stage is allowed."""
import os
import re
import shutil
import struct
import subprocess

import pytest

from helpers import fasta_qual_inputs as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "moira_amd", "csrc")


def build(tmp, *defines):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = os.path.join(str(tmp), "check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "include"), "-I", CSRC] + list(defines) +
                          [os.path.join(ROOT, "tests", "helpers", "fasta_qual_lane_check.cpp"), os.path.join(CSRC, "fastio.cpp"),
                           "-o", exe])
    return exe


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return build(tmp_path_factory.mktemp("fasta_qual_model"))


def pack(c):
    return struct.pack("<32s4q2i", c["name"].encode(), len(c["ftext"]), len(c["qtext"]), c["max_records"], c["out_cap"],
                       int(c["final"]), c["max_len"]) + c["ftext"] + c["qtext"]


def run(exe, tmp, cases):
    fin = os.path.join(str(tmp), "cases.bin")
    with open(fin, "wb") as fh:
        fh.write(struct.pack("<i", len(cases)) + b"".join(pack(c) for c in cases))
    p = subprocess.run([exe, fin], capture_output=True, text=True)
    lines = {}
    for ln in p.stdout.splitlines():
        mt = re.match(r"case (\S+): (taken|back|FAIL)(.*)", ln)
        if mt:
            lines[mt.group(1)] = (mt.group(2), mt.group(3).strip())
    return p.returncode, p.stdout[-3000:] + p.stderr[-3000:], lines


def check(exe, tmp, cases):
    rc, out, lines = run(exe, tmp, cases)
    assert rc == 0 and re.search(r"%d cases, \d+ taken, 0 loads out of bounds, 0 unsupported texts taken, 0 fail" % len(cases), out), out
    assert set(lines) == {c["name"] for c in cases}
    return lines


def fields(s):
    return {k: int(v) for k, v in re.findall(r"(\w+)=(-?\d+)", s)}


def as_host(c, line):
    """A `taken` line against fastio.fasta_qual_index on the same case."""
    w = X.want(c)
    assert w is not None, c["name"]
    out, idx, fc, qc = w
    got = fields(line)
    assert (got["n"], got["fc"], got["qc"], got["used"]) == (len(idx), fc, qc, len(out)), (c["name"], line)


def test_directed_cases_are_the_hosts_or_handed_back_with_their_reason(checker, tmp_path):
    cases = X.directed_cases()
    lines = check(checker, tmp_path, cases)
    for c in cases:
        verdict, rest = lines[c["name"]]
        if c["expect"] is None:
            assert verdict == "taken", (c["name"], rest)
            as_host(c, rest)
        else:
            got = fields(rest)
            assert verdict == "back" and (got["why"], got["which"], got["bad"]) == c["expect"], (c["name"], rest)
    # what the cases are there for
    by = {c["name"]: fields(lines[c["name"]][1]) for c in cases}
    assert by["max_records_cuts"]["n"] == 3 and by["out_cap_cuts"]["n"] == 2 and by["out_cap_exact"]["n"] == 3 and by["out_cap_0"]["n"] == 0
    assert by["not_final_open_line"]["n"] == 3 and by["final_open_line"]["n"] == 4 and by["fewer_in_qual_not_final"]["n"] == 3
    assert by["max_len_3"]["longest"] == 3 and by["tile_edge"]["n"] == 110 and 0 < by["tile_edge_out_cap"]["n"] < 110
    assert by["straddle"]["n"] == 16 and by["straddle"]["longest"] == 90
    # the one refusal the host does not share; everything else that is handed back the host calls unsupported too
    for c in cases:
        if c["expect"] is not None:
            assert (fields(lines[c["name"]][1])["host"] == 0) == (c["name"] == "zeros_0007"), c["name"]


def test_records_of_65535_values_are_the_hosts_or_handed_back_with_their_reason(checker, tmp_path):
    """Quality lines of up to 256 KiB: up to 2,048 steps of a group over a line, every load and store checked (the kernels:
    tests/test_gpu_long_text.py)."""
    cases = X.long_cases()
    lines = check(checker, tmp_path, cases)
    for c in cases:
        verdict, rest = lines[c["name"]]
        if c["expect"] is None:
            assert verdict == "taken", (c["name"], rest)
            as_host(c, rest)
            assert fields(rest)["longest"] == (c["max_len"] or 65535)
        else:
            got = fields(rest)
            assert verdict == "back" and (got["why"], got["which"], got["bad"]) == c["expect"], (c["name"], rest)
            assert (got["host"] == 0) == (c["name"] == "long_zeros_0007"), c["name"]


def test_two_thousand_valid_small_texts_are_all_taken(checker, tmp_path):
    cases = X.fuzz_cases()
    assert len(cases) == 2000
    lines = check(checker, tmp_path, cases)
    assert all(v == "taken" for v, _ in lines.values()), [k for k, (v, _) in lines.items() if v != "taken"][:5]
    for c in cases[::50]:
        as_host(c, lines[c["name"]][1])
    assert sum(fields(r)["n"] for _, r in lines.values()) > 4000


def test_damaged_texts_are_taken_only_as_the_host_takes_them(checker, tmp_path):
    cases = X.damage_cases()
    lines = check(checker, tmp_path, cases)       # (taken: equal to the host's, and never what the host calls unsupported)
    taken = [c for c in cases if lines[c["name"]][0] == "taken"]
    assert 0 < len(taken) < len(cases), len(taken)
    reasons = {fields(r)["why"] for v, r in lines.values() if v == "back"}
    assert {X.TOKEN, X.LENGTH, X.NAMES, X.TRUNCATED} <= reasons, reasons
    for c in taken[::10]:
        as_host(c, lines[c["name"]][1])


def value_cases():
    return [c for c in X.directed_cases() if c["name"].startswith(("value_", "digits_", "zeros_", "tabs"))]


def test_forgetting_the_value_cap_takes_255_and_300(tmp_path):
    exe = build(tmp_path, "-DFA_WRONG_NO_VALUE_CAP")
    cases = value_cases()
    rc, out, lines = run(exe, tmp_path, cases)
    assert rc == 4, out
    for c in cases:
        over = c["name"] in ("value_255", "value_300", "value_999")
        assert (lines[c["name"]][0] == "FAIL") == over, (c["name"], out)


def test_ranking_tokens_by_bytes_fails_every_line_with_a_longer_token(tmp_path):
    exe = build(tmp_path, "-DFA_WRONG_RANK_BY_BYTES")
    cases = [c for c in value_cases() if c["expect"] is None] + [c for c in X.directed_cases() if c["name"] == "straddle"]
    rc, out, lines = run(exe, tmp_path, cases)
    assert rc == 4, out
    for c in cases:
        assert lines[c["name"]][0] == ("taken" if c["name"] == "digits_1" else "FAIL"), (c["name"], out)
