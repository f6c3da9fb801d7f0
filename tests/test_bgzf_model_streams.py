"""tests/golden/bgzf_model_streams.json, the fixture tests/test_gpu_bgzf.py holds k_bgzf_deflate's bytes to, against the host lane
model it was written from (tests/helpers/bgzf_lane_check.cpp, built with -fsanitize=address,undefined and run as a program, as
tests/test_bgzf_lane_model.py does): every entry recomputed, every model stream inflated with zlib, the precondition of every
input of bgzf_inputs.model_inputs() -- what makes it a test of the part it is for -- and the evidence that the fixture tells the
kernel's documented order of look-ups and insertions from two others that round trips cannot see."""
import hashlib
import shutil

import pytest

from helpers import bgzf_inputs as B
from helpers import bgzf_model as M


def build(tmp_path_factory, name, defines=()):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    return M.build(str(tmp_path_factory.mktemp("bgzf_streams") / name), M.SANITIZED + tuple(defines))


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    """({name: [fixture entry per member]}, {name: [the model's dict per member]}) over everything the fixture covers"""
    exe = build(tmp_path_factory, "check")
    return M.compute(exe, str(tmp_path_factory.mktemp("bgzf_streams_run")), M.all_inputs())


def huffman_depth(freq):
    """Depth of the unlimited Huffman tree over the used symbols, built as bz_build_lengths builds it: sorted by (count, symbol),
    two queues, a leaf before an internal node of the same weight."""
    w = sorted(f for f in freq if f)
    m = len(w)
    parent, leaf, node = {}, 0, m
    for _ in range(m - 1):
        pick = []
        for _ in range(2):
            if leaf < m and (node >= len(w) or w[leaf] <= w[node]):
                pick.append(leaf)
                leaf += 1
            else:
                pick.append(node)
                node += 1
        parent[pick[0]] = parent[pick[1]] = len(w)
        w.append(w[pick[0]] + w[pick[1]])
    depth = {len(w) - 1: 0}
    for v in range(len(w) - 2, -1, -1):
        depth[v] = depth[parent[v]] + 1
    return max(depth[v] for v in range(m))


def test_huffman_depth_on_known_trees():
    assert huffman_depth([1, 1]) == 1 and huffman_depth([5, 5, 5, 5]) == 2 and huffman_depth([1] * 286) == 9
    assert huffman_depth([1, 1, 2, 3, 5, 8, 13, 21]) == 7 and huffman_depth([0, 1, 2, 4, 8, 0, 16]) == 4


def test_the_fixture_is_the_model(model):
    entries, _ = model
    fixture = M.load()
    assert list(fixture) == list(entries)
    for name in entries:
        assert fixture[name] == entries[name], name
    with open(M.FIXTURE) as f:
        assert f.read() == M.dumps(entries)                 # (what tests/golden/make_bgzf_model_streams.py writes)
    assert sum(len(v) for v in entries.values()) >= 74 + len(B.model_inputs())


def test_every_model_stream_inflates_to_its_text(model):
    entries, raw = model
    for name, text in M.all_inputs():
        ms = B.members(text)
        assert len(ms) == len(raw[name]) == len(entries[name])
        for m, g, e in zip(ms, raw[name], entries[name]):
            assert B.inflate_raw(g["stream"]) == m, name
            assert g["oob"] == 0 and e["literals"] + e["matched"] == e["n"] == len(m)
            first = g["stream"][0]
            assert (first == 1) if e["btype"] == M.STORED else (first & 7 == 1 | e["btype"] << 1), name


def only(model, name):
    entries, raw = model
    assert len(entries[name]) == 1
    return dict(B.model_inputs())[name], entries[name][0], raw[name][0]


def test_buffer_nearly_full(model):
    text, e, _ = only(model, "buffer_nearly_full")
    assert len(text) == B.DATA and e["btype"] == M.DYNAMIC
    assert 0.995 * (e["n"] + 5) <= e["bytes"] < e["n"] + 5
    assert e["bytes"] > 4 * (16384 - 128)                   # the emit phase reaches the last 128 of its 16,384 words


def test_codes_of_15_bits(model):
    _, e, g = only(model, "codes_of_15_bits")
    assert e["btype"] == M.DYNAMIC and max(g["ll"]) == 15 and e["n"] == 36 ** 3 + 4 * sum(B.FIB16)


def test_length_limit_binds(model, tmp_path_factory):
    """The unlimited tree over the model's own literal/length histogram is deeper than 15: bz_build_lengths halves."""
    text, e, g = only(model, "length_limit_binds")
    exe = build(tmp_path_factory, "check_histograms", ("-DBZ_CHECK_HISTOGRAMS",))
    h, = M.run(exe, str(tmp_path_factory.mktemp("bgzf_streams_hist")), [("member", text)], histograms=True)
    assert h["stream"] == g["stream"]                       # (the switch adds the counts and changes nothing)
    assert sum(h["ll_freq"]) == e["literals"] + e["matches"] + 1 and sum(h["d_freq"]) == e["matches"]
    assert huffman_depth(h["ll_freq"]) > 15
    assert e["btype"] == M.DYNAMIC and max(g["ll"]) <= 15


def test_code_length_limit_binds(model):
    """The unlimited tree over the counts of the code lengths in the header is deeper than 7: the third tree is halved."""
    text, e, g = only(model, "code_length_limit_binds")
    assert all(text.find(text[p:p + 3]) == p for p in range(len(text) - 2)) and e["matches"] == 0
    counts = [0] * 16
    for bits in list(g["ll"][:g["hlit"]]) + list(g["dl"][:g["hdist"]]):
        counts[bits] += 1
    assert [counts[bits] for bits in sorted(B.CL_LIMIT_SHAPE)] == [v + (bits == 15) for bits, v in sorted(B.CL_LIMIT_SHAPE.items())]
    assert huffman_depth(counts) > 7
    assert e["btype"] == M.DYNAMIC and max(g["cl"]) == 7


def test_period_members(model):
    """Every step but the first is one match per 258 positions and the same two buckets for all of them; period 5 is above
    BZ_DIRECT, so its first step finds nothing (the tables are empty until the step's insertions) and is all literals."""
    _, e, _ = only(model, "period2_member")
    assert (e["n"], e["literals"], e["matches"], e["matched"]) == (B.DATA, 2, 254, B.DATA - 2)
    _, e, _ = only(model, "period5_member")
    assert (e["n"], e["literals"], e["matches"], e["matched"]) == (B.DATA, 256, 253, B.DATA - 256)


def test_match_258_ends_the_member(model):
    text, e, _ = only(model, "match_258_ends_the_member")
    n = len(text)
    assert text[n - 258:] == text[n - 516:n - 258]
    assert all(text.find(text[p:p + 3]) == p for p in range(n - 258))      # nothing before the last 258 bytes starts a repeat,
    assert (e["matches"], e["matched"], e["literals"]) == (1, 258, n - 258)  # so the one match, of 258, is the last token
    assert e["literals"] + e["matched"] == n


@pytest.mark.parametrize("switch", ["BZ_CHECK_INSERT_FIRST", "BZ_CHECK_SMALLEST_WINS"])
def test_the_fixture_tells_another_order_apart(switch, tmp_path_factory):
    """A model whose insertions of a step precede its look-ups, or in which the smallest position of a step wins a bucket, still
    writes valid streams of every text, and different ones: the digests see what the round trip cannot."""
    exe = build(tmp_path_factory, "check_" + switch.lower(), ("-D" + switch,))
    inputs = list(B.model_inputs()) + list(B.named_inputs())
    _, raw = M.compute(exe, str(tmp_path_factory.mktemp("bgzf_streams_variant")), inputs)
    fixture, differ = M.load(), []
    for name, text in inputs:
        for k, (m, g) in enumerate(zip(B.members(text), raw[name])):
            assert B.inflate_raw(g["stream"]) == m, name
            if hashlib.sha256(g["stream"]).hexdigest() != fixture[name][k]["sha256"]:
                differ.append((name, k))
    assert differ, switch
