"""The device compressor's per-lane code on the host (moira_amd/csrc/mpb_bgzf_lane.inc through tests/helpers/bgzf_lane_check.cpp,
built with -fsanitize=address,undefined and run as a program): whole members go through it in the kernel's order with checked
loads, zlib inflates what it wrote, and the Huffman length builder runs alone on adversarial histograms.  Every tree's Kraft sum
is checked.  The kernels themselves: tests/test_gpu_bgzf.py."""
import shutil
from fractions import Fraction

import pytest

from helpers import bgzf_inputs as B
from helpers import bgzf_model as M

STORED, FIXED, DYNAMIC = M.STORED, M.FIXED, M.DYNAMIC


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    return M.build(str(tmp_path_factory.mktemp("bgzf_model") / "check"), M.SANITIZED)


run = M.run


def kraft(lens):
    return sum(Fraction(1, 2 ** l) for l in lens if l)


def check_member(text, g):
    assert B.inflate_raw(g["stream"]) == text
    assert g["oob"] == 0 and g["literals"] + g["matched"] == len(text)
    assert len(g["stream"]) <= len(text) + 5
    # the trees as built: complete codes within their limits
    assert kraft(g["ll"]) == 1 and max(g["ll"]) <= 15 and g["ll"][256] > 0
    assert kraft(g["dl"]) == 1 and max(g["dl"]) <= 15
    if g["btype"] == DYNAMIC:
        assert kraft(g["cl"]) == 1 and max(g["cl"]) <= 7 and not any(g["cl"][16:])


def test_directed_members_inflate_with_zlib(checker, tmp_path):
    cases = [(name, m) for name, text in B.named_inputs() for m in B.members(text)]
    got = run(checker, str(tmp_path), [("member", m) for _, m in cases])
    by = {}
    for (name, m), g in zip(cases, got):
        check_member(m, g)
        by.setdefault(name, []).append(g)
    assert by["random_member"][0]["btype"] == STORED
    assert by["random_1000"][0]["btype"] in (STORED, FIXED)
    # a run of one byte: distance 1, overlapping copies at the cap of 258 -- one literal, then matches only
    run1 = by["one_byte_member"][0]
    assert run1["literals"] == 1 and run1["matches"] == -(-(B.DATA - 1) // 258) and len(run1["stream"]) < 400
    assert by["no_repeat"][0]["matches"] == 0 and by["no_repeat"][0]["btype"] == DYNAMIC and by["no_repeat"][0]["hdist"] >= 1
    # the largest legal distance is taken, the first illegal one is not (random bytes repeat nowhere else: a bucket of the hash
    # table that a later position took over costs a few literals, so most, not all, of the second period is matched)
    assert by["period32768"][0]["matched"] >= (B.DATA - 32768) // 2
    assert by["period32769"][0]["matched"] < 3000
    # the second member repeats the end of the first and nothing of its own
    assert by["repeat_across_border"][1]["matched"] < 100
    for period in (3, 64, B.STEP - 1, B.STEP + 1):
        assert by["period%d" % period][0]["matched"] >= 5000 - 3 * max(period, B.STEP), period
    assert by["all_bytes_twice"][0]["matched"] >= 250
    end = by["min_match_at_end"][0]
    assert (end["matches"], end["matched"], end["literals"]) == (1, 3, 703)


def test_golden_texts_compress_without_a_stored_member(checker, tmp_path):
    """Any Huffman code over a FASTQ alphabet is smaller than the text: no member of the golden renderings is stored."""
    for text in B.golden_renderings():
        ms = B.members(text)
        got = run(checker, str(tmp_path), [("member", m) for m in ms])
        for m, g in zip(ms, got):
            check_member(m, g)
            assert g["btype"] != STORED
        assert sum(len(g["stream"]) + 26 for g in got) < len(text)


def test_fuzz_members_inflate_with_zlib(checker, tmp_path):
    ms = [B.fuzz_member(k) for k in range(20)]
    for m, g in zip(ms, run(checker, str(tmp_path), [("member", m) for m in ms])):
        check_member(m, g)


def test_length_builder_on_adversarial_histograms(checker, tmp_path):
    fib = [1, 1]
    while len(fib) < 40:
        fib.append(fib[-1] + fib[-2])
    hists = [
        (15, fib[:30] + [0] * 256),                     # Fibonacci counts: an unlimited tree is 29 deep
        (15, [0] * 100 + fib[:40] + [0] * 146),
        (7, fib[:16]),                                  # the code-length code's limit
        (7, [3 ** k for k in range(16)]),
        (15, [0] * 65 + [9] + [0] * 220),               # a single used symbol: a second one is added
        (15, [0] * 30),                                 # no match at all: zero distance codes
        (15, [0] * 7 + [5] + [0] * 22),                 # exactly one distance code
        (15, [5] + [0] * 29),
        (15, [1] * 286),
        (15, [2 ** 16 - 1] * 285 + [1]),
        (15, list(range(1, 287))),
    ]
    got = run(checker, str(tmp_path), [("hist", limit, h) for limit, h in hists])
    for (limit, h), lens in zip(hists, got):
        lens = list(lens)
        assert kraft(lens) == 1, (limit, h[:8])
        assert max(lens) <= limit
        used = [k for k, f in enumerate(h) if f]
        assert all(lens[k] > 0 for k in used)
        assert sum(1 for l in lens if l) == max(2, len(used))
        for a in used:                                  # a more frequent symbol never has the longer code
            for b in used:
                if h[a] > h[b]:
                    assert lens[a] <= lens[b], (a, b)
    # where the limit does not bind, the lengths are Huffman's: the cost equals the optimum
    import heapq
    h = list(range(1, 287))
    heap = list(h)
    heapq.heapify(heap)
    cost = 0
    while len(heap) > 1:
        s = heapq.heappop(heap) + heapq.heappop(heap)
        cost += s
        heapq.heappush(heap, s)
    assert sum(f * l for f, l in zip(h, got[-1])) == cost
