"""The device FASTQ indexer's lane code on the host (moira_amd/csrc/mpb_index_lane.inc through
tests/helpers/fastq_index_check.cpp, built with -fsanitize=address,undefined together with csrc/fastio.cpp and run as a program;
nothing is preloaded): the directed texts of tests/helpers/fastq_index_texts.py and a seeded fuzz go through the four kernels'
steps with 256 lane states (four waves of 64) in lockstep and checked loads and stores.  The program compares rows, n, consumed
and bad_kind with mio_fastq_index itself; here its verdicts are checked again against fastio.index.  The kernels themselves:
tests/test_gpu_fastq_index.py."""
import os
import shutil
import struct
import subprocess

import pytest

from helpers import fastq_index_texts as X
from moira_amd import fastio as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_UNSUPPORTED = -2


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("fastq_index_model") / "check")
    csrc = os.path.join(ROOT, "moira_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "include"), "-I", csrc,
                           os.path.join(ROOT, "tests", "helpers", "fastq_index_check.cpp"), os.path.join(csrc, "fastio.cpp"), "-o", exe])
    return exe


def run(exe, tmp, cases, max_len=0, expect_exit=0):
    """cases: [(name, text, final, max_records)] -> [dict]."""
    blob = [struct.pack("<i", len(cases))]
    for _, text, final, max_records in cases:
        blob += [struct.pack("<2q2i", len(text), max_records, final, max_len), text]
    fin, fout = os.path.join(tmp, "cases.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as f:
        f.write(b"".join(blob))
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert r.returncode == expect_exit, r.stdout[-2000:] + r.stderr[-4000:]
    assert " 0 loads or stores out of bounds, 0 differ from mio_fastq_index, 0 unsupported texts taken" in r.stdout, r.stdout
    raw = open(fout, "rb").read()
    assert len(raw) == 40 * len(cases)
    keys = ("why", "bad_kind", "n", "consumed", "longest", "host_rc", "pad")
    return [dict(zip(keys, struct.unpack_from("<2i3q2i", raw, 40 * k))) for k in range(len(cases))]


def host(text, final, max_records):
    try:
        idx, consumed, bad = F.index(text, bool(final), min(max_records, len(text) // 4 + 1))
    except F.Unsupported:
        return None
    return len(idx), consumed, bad.kind if bad is not None else 0


def check_taken(cases, got):
    for (name, text, final, max_records), g in zip(cases, got):
        assert g["why"] == 0, (name, g)
        assert (g["n"], g["consumed"], g["bad_kind"]) == host(text, final, max_records), name


def test_the_helper_texts_are_what_they_claim():
    names = [c[0] for c in X.directed() + X.handed_back()]
    assert len(set(names)) == len(names)
    by = {c[0]: c for c in X.directed()}
    assert by["nl_ends_tile/final"][1][X.T - 1:X.T] == b"\n" and by["nl_first_of_tile/final"][1][X.T:X.T + 1] == b"\n"
    assert by["cr_ends_tile/final"][1][X.T - 1:X.T + 1] == b"\r\n"
    assert [len(by["bytes%d/final" % s][1]) for s in (X.T - 1, X.T, X.T + 1)] == [X.T - 1, X.T, X.T + 1]
    kinds = {host(by["%s_middle/final" % k][1], 1, X.BIG)[2] for k in ("empty_seq", "empty_qual", "mismatch")}
    assert kinds == {F.REC_EMPTY_SEQ, F.REC_EMPTY_QUAL, F.REC_LENGTH_MISMATCH}
    for name, text, final, max_records, why in X.handed_back():
        if "behind" not in name:
            assert host(text, final, max_records) is None, name      # the host calls these unsupported itself
    for name, text, final, max_records in X.not_looked_at() + X.fuzz(200):
        assert host(text, final, max_records) is not None, name


def test_directed_texts_equal_the_host_index(checker, tmp_path):
    cases = X.directed()
    check_taken(cases, run(checker, str(tmp_path), cases))


def test_records_of_65535_bases_equal_the_host_index(checker, tmp_path):
    """Tiles without a newline, lines over four tiles (the kernels: tests/test_gpu_long_text.py)."""
    cases = X.long_reads()
    got = run(checker, str(tmp_path), cases)
    check_taken(cases, got)
    assert max(g["longest"] for g in got) == 65535
    got = run(checker, str(tmp_path), cases[:2], max_len=40000)
    check_taken(cases[:2], got)
    assert max(g["longest"] for g in got) == 40000


def test_descriptors_with_max_len(checker, tmp_path):
    cases = X.endings() + X.headers()
    got = run(checker, str(tmp_path), cases, max_len=3)
    check_taken(cases, got)
    assert max(g["longest"] for g in got) == 3


def test_handed_back_with_the_right_reason(checker, tmp_path):
    cases = X.handed_back()
    got = run(checker, str(tmp_path), [c[:4] for c in cases])
    for (name, text, final, max_records, why), g in zip(cases, got):
        assert g["why"] == why, (name, g)


def test_every_fuzz_text_is_taken(checker, tmp_path):
    cases = X.fuzz()
    assert len(cases) == 2000 and max(len(c[1]) for c in cases) <= 4096
    got = run(checker, str(tmp_path), cases)
    assert all(g["why"] == 0 and g["host_rc"] == 0 for g in got)
    check_taken(cases[::20], got[::20])


def test_damaged_texts_are_taken_only_as_the_host_indexes_them(checker, tmp_path):
    """Seeded damage: a '\\r' or a byte >= 0x80 dropped anywhere into a valid text.  The program fails the run when a text the
    host calls unsupported is taken or a taken one differs; some must still be taken (damage behind the last newline)."""
    import numpy as np
    rng = np.random.default_rng(5)
    base = b"".join(X.records(8, 23))
    cases = []
    for k in range(300):
        at = int(rng.integers(0, len(base) + 1))
        cut = int(rng.integers(at, len(base) + 1))
        cases.append(("damage%d" % k, base[:at] + (b"\r" if k % 2 else b"\xe2") + base[at:cut], k % 3 == 0, X.BIG if k % 5 else 3))
    got = run(checker, str(tmp_path), cases)
    taken = sum(g["why"] == 0 for g in got)
    assert 0 < taken < len(cases)
    for c, g in zip(cases, got):
        if g["host_rc"] == E_UNSUPPORTED:
            assert g["why"] in (1, 2), c[0]
