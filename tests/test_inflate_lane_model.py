"""The device inflater's lane code on the host (moira_amd/csrc/mpb_inflate_lane.inc through tests/helpers/inflate_lane_check.cpp,
built with -fsanitize=address,undefined and run as a program): every input of tests/helpers/inflate_inputs.py goes through
bi_member with 64 lane states in lockstep and checked loads and stores.  Valid members must come out as the host decoder's text,
invalid ones with their reason, and nothing the host rejects may be taken.  The helper's own inputs are checked against zlib
here as well.  The kernel itself: tests/test_gpu_bgzf_inflate.py."""
import os
import shutil
import struct
import subprocess
import zlib

import pytest

from helpers import inflate_inputs as I

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("why", "iterations", "cap", "oob", "differ", "stored", "fixed", "dynamic", "literals", "matches", "matched", "longest")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("inflate_model") / "check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "moira_amd", "csrc"),
                           os.path.join(ROOT, "tests", "helpers", "inflate_lane_check.cpp"), "-o", exe])
    return exe


def run(exe, tmp, cases):
    """cases: [(stream, out_len, lead, shift)] -> [dict]."""
    blob = [struct.pack("<i", len(cases))]
    for stream, out_len, lead, shift in cases:
        blob += [struct.pack("<4i", len(stream), out_len, lead, shift), stream]
    fin, fout = os.path.join(tmp, "cases.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as f:
        f.write(b"".join(blob))
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert " 0 loads out of bounds, 0 lane states differ, 0 over the cap" in r.stdout, r.stdout
    raw, pos, out = open(fout, "rb").read(), 0, []
    for _ in cases:
        vals = struct.unpack_from("<13i", raw, pos)
        pos += 52
        g = dict(zip(FIELDS, vals))
        g["text"] = raw[pos:pos + vals[12]]
        pos += vals[12]
        out.append(g)
    assert pos == len(raw)
    return out


def inflate_raw(stream):
    d = zlib.decompressobj(-15)
    text = d.decompress(stream)
    assert d.eof and not d.unused_data
    return text


def test_the_helpers_valid_members_inflate_with_zlib():
    for name, stream, text, _ in I.crafted_valid() + I.zlib_members() + I.fuzz_members():
        assert inflate_raw(stream) == text, name
        assert len(text) <= 65536 and len(I.frame(stream, text)) <= 65536, name
    names = [n for n, _, _, _ in I.crafted_valid()]
    assert len(set(names)) == len(names)
    blob = I.frame(b"\x03\0", b"", extra=b"ZZ\x03\0abc")
    assert I.parse(blob) == (25, 2, 0, 0)


def check_valid(cases, got):
    for k, ((name, stream, text, blocks), g) in enumerate(zip(cases, got)):
        assert g["why"] == I.OK, (name, g)
        assert g["text"] == text, name
        assert g["iterations"] <= g["cap"], name
        stored_bytes = len(text) - g["literals"] - g["matched"]              # literals + matched bytes + stored bytes = text bytes
        assert stored_bytes >= 0 and (g["stored"] > 0 or stored_bytes == 0), name
        if blocks is not None:
            assert (g["stored"], g["fixed"], g["dynamic"]) == blocks, (name, g)


def test_crafted_valid_members(checker, tmp_path):
    cases = I.crafted_valid()
    got = run(checker, str(tmp_path), [(s, len(t), 18 + k % 5, k % 16) for k, (_, s, t, _) in enumerate(cases)])
    check_valid(cases, got)
    by = {c[0]: g for c, g in zip(cases, got)}
    assert by["dist_ladder_15bit"]["longest"] == 15
    assert by["match258_distance1"]["matches"] == 1 and by["match258_distance1"]["matched"] == 258
    assert by["single_1bit_distance_code"]["matched"] == 288
    assert by["literal_only_hdist1_len0"]["matches"] == 0
    assert by["end_marker"]["literals"] == 0 and by["end_marker"]["text"] == b""


def test_zlib_members_at_every_setting(checker, tmp_path):
    cases = I.zlib_members()
    got = run(checker, str(tmp_path), [(s, len(t), 18 + (3 * k) % 16, (5 * k) % 16) for k, (_, s, t, _) in enumerate(cases)])
    check_valid(cases, got)
    by = {c[0]: g for c, g in zip(cases, got)}
    assert by["fibonacci"]["longest"] == 15 and by["fibonacci"]["matches"] == 0
    assert by["memlevel1"]["dynamic"] > 30
    assert by["level0"]["literals"] == 0 and by["level0"]["matched"] == 0
    for lv in (1, 4, 9):
        assert by["level%d" % lv]["longest"] >= 9


def test_fuzz_members(checker, tmp_path):
    cases = I.fuzz_members()
    got = run(checker, str(tmp_path), [(s, len(t), 18, k % 16) for k, (_, s, t, _) in enumerate(cases)])
    check_valid(cases, got)


def test_invalid_members_are_handed_back_with_their_reason(checker, tmp_path):
    """The lane code sees the stream and ISIZE; header and CRC defects are the rows' and the host entry's (other tests)."""
    cases = [(n, m, why) for n, m, why in I.crafted_invalid() if why not in (I.HEADER, I.CRC)]
    args = []
    for _, m, _ in cases:
        off, slen, _, isize = I.parse(m)
        args.append((m[off:off + slen], isize, off, 3))
    got = run(checker, str(tmp_path), args)
    host = I.host_inflate([m for _, m, _ in cases])
    for (name, m, why), g, (htext, herr) in zip(cases, got, host):
        assert g["why"] == why, (name, g)
        assert htext is None, name                           # (what the host rejects is never taken: the rule itself)
        assert g["text"] == b""


def test_whatever_the_host_rejects_is_handed_back(checker, tmp_path):
    """Seeded damage to valid streams: one byte changed, or the tail cut.  Taken only if the host takes it, with equal bytes."""
    import numpy as np
    rng = np.random.default_rng(77)
    base = [c for c in I.zlib_members() if len(c[1]) < 12000][:6] + I.crafted_valid()[:4]
    members, args = [], []
    for name, stream, text, _ in base:
        for _ in range(12):
            s = bytearray(stream)
            if rng.random() < 0.3 and len(s) > 4:
                s = s[:int(rng.integers(1, len(s)))]
            else:
                s[int(rng.integers(0, len(s)))] ^= 1 << int(rng.integers(0, 8))
            members.append(I.frame(bytes(s), text))
            args.append((bytes(s), len(text), 18, 0))
    got = run(checker, str(tmp_path), args)
    taken = 0
    for m, g, (htext, herr) in zip(members, got, I.host_inflate(members)):
        if g["why"] == I.OK and zlib.crc32(g["text"]) == I.parse(m)[2]:          # (the host entry's CRC check)
            assert htext is not None and htext == g["text"]
            taken += 1
    assert taken < len(members)
