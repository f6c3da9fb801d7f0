"""The pairing kernels' lane code on the host (moira_amd/csrc/mpb_pair_lane.inc through tests/helpers/pair_lane_check.cpp, built
with -fsanitize=address,undefined together with csrc/mpb_hostonly.cpp and csrc/fastio.cpp and run as a program; nothing is
preloaded): 256 lane states in lockstep, every load checked against the two index arrays and the two validated header ranges.
The program compares with mpb_pair_rows (byte for byte on the rows), mio_first_header_mismatch, the host's class and list
construction and rec_cap = the largest need + 8; here its verdicts are checked again against fastio.  Two sensitivity builds
must fail named cases.  The kernels themselves: tests/test_gpu_pair_index.py."""
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

from helpers import pair_index_inputs as X
from moira_amd import fastio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "moira_amd", "csrc")
EDGES = (1, 64, 65, 128, 256, 257, 384, 385)
TOKEN_LENGTHS = (1, 15, 16, 17, 300)
COUNTS = (0, 1, 63, 64, 65, 255, 256, 257, 1000)


def class_caps():
    """k_lds_class[] as mpb_contig.cpp holds it: nothing of the table is restated here."""
    lds_max = int(re.search(r"#define MPB_CONTIG_LDS_MAX (\d+)", open(os.path.join(CSRC, "mpb_contig_args.h")).read()).group(1))
    src = open(os.path.join(CSRC, "mpb_contig.cpp")).read()
    return [lds_max if t.strip() == "MPB_CONTIG_LDS_MAX" else int(t) for t in re.search(r"k_lds_class\[\] = \{([^}]*)\}", src).group(1).split(",")]


def build(tmp, *defines):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = os.path.join(str(tmp), "check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "include"), "-I", CSRC] + list(defines) +
                          [os.path.join(ROOT, "tests", "helpers", "pair_lane_check.cpp"), os.path.join(CSRC, "mpb_hostonly.cpp"),
                           os.path.join(CSRC, "fastio.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return build(tmp_path_factory.mktemp("pair_model"))


def token(i, length):
    """A header token of exactly `length` bytes that names pair i."""
    s = ("%d" % i).encode()
    return (s + b"_" * length)[:length] if length >= len(s) else s[-length:]


def texts(lengths, tokens=None, rtokens=None):
    """The two files of pairs of the given (l1, l2) and their host indexes."""
    tokens = tokens or [("r%06d" % i).encode() for i in range(len(lengths))]
    rtokens = rtokens or tokens
    f = X.fastq_text([(tokens[i], b"A" * l1, b"I" * l1) for i, (l1, _) in enumerate(lengths)])
    r = X.fastq_text([(rtokens[i], b"C" * l2, b"5" * l2) for i, (_, l2) in enumerate(lengths)])
    n = len(lengths)
    return f, fastio.index(f, True, n)[0].copy(), r, fastio.index(r, True, n)[0].copy()


def case(name, f, fidx, r, ridx, m=None, maxabs=2, take=1):
    return dict(name=name, f=f, fidx=np.ascontiguousarray(fidx, np.int64), r=r, ridx=np.ascontiguousarray(ridx, np.int64),
                m=min(len(fidx), len(ridx)) if m is None else m, maxabs=maxabs, take=take)


def run(exe, tmp, cases):
    caps = class_caps()
    blob = [struct.pack("<i", len(cases))]
    for c in cases:
        blob += [struct.pack("<32s5q4i16i", c["name"].encode(), len(c["fidx"]), len(c["ridx"]), c["m"], len(c["f"]), len(c["r"]), c["maxabs"],
                             c["take"], len(caps), 0, *(caps + [0] * (16 - len(caps)))),
                 c["fidx"].tobytes(), c["ridx"].tobytes(), c["f"], c["r"]]
    fin = os.path.join(str(tmp), "cases.bin")
    with open(fin, "wb") as fh:
        fh.write(b"".join(blob))
    p = subprocess.run([exe, fin], capture_output=True, text=True)
    lines = {}
    for ln in p.stdout.splitlines():
        mt = re.match(r"case (\S+): (ok|refused|FAIL)(.*)", ln)
        if mt:
            d = dict(kv.split("=") for kv in mt.group(3).split() if "=" in kv) if mt.group(2) != "FAIL" else {"what": mt.group(3)}
            lines[mt.group(1)] = (mt.group(2), d)
    return p.returncode, p.stdout + p.stderr[-3000:], lines


def check(exe, tmp, cases):
    rc, out, lines = run(exe, tmp, cases)
    assert rc == 0 and "%d cases, 0 loads out of bounds, 0 fail" % len(cases) in out, out
    assert set(lines) == {c["name"] for c in cases}
    return lines


def length_cases():
    rng = np.random.default_rng(41)
    lengths = [(a, b) for a in EDGES for b in EDGES] + [(int(a), int(b)) for a, b in rng.integers(1, 401, (200, 2))]
    tokens = [token(i, TOKEN_LENGTHS[i % len(TOKEN_LENGTHS)]) for i in range(len(lengths))]
    return lengths, tokens


def mismatch_cases():
    lengths = [(100 + i % 50, 90 + i % 70) for i in range(300)]
    out = []
    for at in (0, 100, 299):
        for how in ("length", "last_byte"):
            tokens = [token(i, TOKEN_LENGTHS[i % len(TOKEN_LENGTHS)]) for i in range(300)]
            rtokens = list(tokens)
            rtokens[at] = tokens[at] + b"x" if how == "length" else tokens[at][:-1] + bytes([tokens[at][-1] ^ 1])
            out.append((at, case("mis_%s_%d" % (how, at), *texts(lengths, tokens, rtokens))))
    return out


def count_cases():
    rng = np.random.default_rng(9)
    out = []
    for n in COUNTS:
        lengths = [((30, 150, 250, 384, 400)[int(a)], (40, 140, 251, 380, 10)[int(b)]) for a, b in rng.integers(0, 5, (n, 2))]
        out.append(case("count_%d" % n, *texts(lengths)))
    return out


def test_every_length_edge_reaches_every_class(checker, tmp_path):
    """Every length pair on the edges and 200 random ones in 1..400, header tokens of 1, 15, 16, 17 and 300 bytes: all ten classes
    and class -1 occur, rows / classes / lists / rec_cap are the host's."""
    lengths, tokens = length_cases()
    f, fidx, r, ridx = texts(lengths, tokens)
    got = check(checker, tmp_path, [case("edges", f, fidx, r, ridx)])["edges"]
    per_class = [int(v) for v in got[1]["classes"].split(",")]
    assert got[0] == "ok" and len(per_class) == 10 and min(per_class) > 0
    longer = sum(a > 384 or b > 384 for a, b in lengths)
    assert longer > 0 and sum(per_class) == len(lengths) - longer
    assert int(got[1]["rec_cap"]) == int((fidx[:, 1] + 2 * (fidx[:, 3] + ridx[:, 3])).max()) + 8
    assert int(got[1]["mismatch"]) == -1 == fastio.first_header_mismatch(f, fidx, r, ridx)


def test_the_gpu_test_pairs_all_have_a_class(checker, tmp_path):
    """The 600 pairs tests/test_gpu_pair_index.py sends through all ten classes: every one has a class on the host, so the
    pairs that test counts as handed back are exactly the ones it damages."""
    pairs = X.class_pairs()
    f, r = X.pair_texts(pairs)
    fidx, ridx = fastio.index(f, True, 600)[0], fastio.index(r, True, 600)[0]
    got = check(checker, tmp_path, [case("gpu_pairs", f, fidx, r, ridx)])["gpu_pairs"]
    per_class = [int(v) for v in got[1]["classes"].split(",")]
    assert min(per_class) > 0 and sum(per_class) == 600


def test_header_mismatches(checker, tmp_path):
    cases = mismatch_cases()
    got = check(checker, tmp_path, [c for _, c in cases])
    for at, c in cases:
        assert fastio.first_header_mismatch(c["f"], c["fidx"], c["r"], c["ridx"]) == at
        assert got[c["name"]][0] == "ok" and (int(got[c["name"]][1]["mismatch"]), int(got[c["name"]][1]["built"])) == (at, at)


def test_pair_counts_across_wave_and_workgroup_borders(checker, tmp_path):
    got = check(checker, tmp_path, count_cases())
    for n in COUNTS:
        assert got["count_%d" % n][0] == "ok" and int(got["count_%d" % n][1]["built"]) == n


def test_a_call_that_takes_no_pair_and_the_score_predicate(checker, tmp_path):
    lengths = [(100 + i, 120 + i) for i in range(80)]
    t = texts(lengths)
    got = check(checker, tmp_path, [case("take_0", *t, take=0), case("maxabs_100", *t, maxabs=100), case("maxabs_30000", *t, maxabs=30000)])
    assert got["take_0"][1]["classes"] == ",".join(["0"] * 10) == got["maxabs_30000"][1]["classes"]
    listed = sum(int(v) for v in got["maxabs_100"][1]["classes"].split(","))
    assert listed == sum((a + b + 2) * 100 < 30000 for a, b in lengths) and 0 < listed < 80


def damaged():
    lengths = [(100 + i, 90 + i) for i in range(50)]
    f, fidx, r, ridx = texts(lengths)
    out = []
    def add(name, which, col, value, row=20):
        a, b = fidx.copy(), ridx.copy()
        (a, b)[which][row, col] = value(int((a, b)[which][row, col]))
        out.append(case(name, f, a, r, b))
    for which in (0, 1):
        w = "fr"[which]
        for col in (0, 2, 4):
            add("neg_off_%s%d" % (w, col), which, col, lambda v: -1)
        add("neg_len_%s" % w, which, 3, lambda v: -5)
        add("neg_hdr_len_%s" % w, which, 1, lambda v: -1)
        add("len_mismatch_%s" % w, which, 5, lambda v: v + 1)
        add("len_2_31_%s" % w, which, 3, lambda v: 1 << 31)
        add("hdr_len_2_31_%s" % w, which, 1, lambda v: 1 << 31)
        add("hdr_past_%s" % w, which, 0, lambda v: len((f, r)[which]) - 3)
        add("off_huge_%s" % w, which, 2, lambda v: (1 << 63) - 1)
    # a line that ends one byte past the text
    for which in (0, 1):
        for col in (2, 4):
            add("one_past_%s%d" % ("fr"[which], col), which, col, lambda v: len((f, r)[which]) - int((fidx, ridx)[which][49, 3]) + 1, row=49)
    return f, fidx, r, ridx, out


def test_damaged_index_rows_are_refused_without_a_load_out_of_bounds(checker, tmp_path):
    f, fidx, r, ridx, cases = damaged()
    # (the "one past" rows must really end one byte past their text, or lie inside it by no more)
    for c in cases:
        if c["name"].startswith("one_past"):
            which, col = "fr".index(c["name"][9]), int(c["name"][10])
            idx, text = (c["fidx"], c["ridx"])[which], (c["f"], c["r"])[which]
            assert idx[49, col] + idx[49, 3] > len(text)
    got = check(checker, tmp_path, cases)
    for c in cases:
        row = 49 if c["name"].startswith("one_past") else 20
        assert got[c["name"]][0] == "refused" and int(got[c["name"]][1]["rowfail"]) == row, (c["name"], got[c["name"]])
    # a damaged row behind a header mismatch is never looked at by the call: the pairs before the mismatch are built
    rt = [("r%06d" % i).encode() for i in range(50)]
    rt[10] = b"other"
    f2, fidx2, r2, ridx2 = texts([(100 + i, 90 + i) for i in range(50)], None, rt)
    fidx2[20, 2] = -1
    got = check(checker, tmp_path, [case("behind_mismatch", f2, fidx2, r2, ridx2)])["behind_mismatch"]
    assert got[0] == "ok" and (int(got[1]["mismatch"]), int(got[1]["built"]), int(got[1]["rowfail"])) == (10, 10, 20)


def test_a_rank_off_by_one_at_a_wave_border_fails_the_lists(tmp_path):
    exe = build(tmp_path, "-DPAIR_CHECK_WRONG_RANK")
    rc, out, lines = run(exe, tmp_path, count_cases())
    assert rc == 4, out
    for n in COUNTS:
        assert lines["count_%d" % n][0] == ("FAIL" if n > 64 else "ok"), (n, out)


def test_a_header_compare_that_stops_one_byte_early_misses_the_last_byte(tmp_path):
    exe = build(tmp_path, "-DPAIR_CHECK_SHORT_HDR")
    cases = mismatch_cases()
    rc, out, lines = run(exe, tmp_path, [c for _, c in cases])
    assert rc == 4, out
    for _, c in cases:
        assert lines[c["name"]][0] == ("FAIL" if "last_byte" in c["name"] else "ok"), (c["name"], out)
