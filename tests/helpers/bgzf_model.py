"""The host lane model of k_bgzf_deflate (tests/helpers/bgzf_lane_check.cpp over moira_amd/csrc/mpb_bgzf_lane.inc) as a program:
building it, running members through it, and the fixture of its results, tests/golden/bgzf_model_streams.json (per input name
and member: n, btype, the stream's length and SHA-256, literals, matches, matched).  The fixture is written by
tests/golden/make_bgzf_model_streams.py, recomputed by tests/test_bgzf_model_streams.py and compared with the device's bytes by
tests/test_gpu_bgzf.py, which needs no compiler for it."""
import hashlib
import json
import os
import struct
import subprocess

import numpy as np

from helpers import bgzf_inputs as B

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
FIXTURE = os.path.join(ROOT, "tests", "golden", "bgzf_model_streams.json")
STORED, FIXED, DYNAMIC = 0, 1, 2
SANITIZED = ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined")
KEYS = ("n", "btype", "bytes", "sha256", "literals", "matches", "matched")
GOLDEN_NAMES = ("golden_fastq", "golden_fasta", "golden_qual")


def build(exe, flags=("-O2",)):
    subprocess.check_call(["g++", *flags, "-std=c++17", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "moira_amd", "csrc"),
                           os.path.join(ROOT, "tests", "helpers", "bgzf_lane_check.cpp"), "-o", exe])
    return exe


def run(exe, tmp, cases, histograms=False):
    """cases: [("member", bytes) | ("hist", limit, counts)] -> [dict | code lengths]; histograms: exe was built with
    -DBZ_CHECK_HISTOGRAMS and every member's dict has its literal/length and distance counts."""
    blob = [struct.pack("<i", len(cases))]
    for c in cases:
        if c[0] == "member":
            blob += [struct.pack("<ii", 0, len(c[1])), c[1]]
        else:
            blob += [struct.pack("<iii", 1, len(c[2]), c[1]), np.asarray(c[2], np.uint32).tobytes()]
    fin, fout = os.path.join(tmp, "cases.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as f:
        f.write(b"".join(blob))
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert " 0 loads out of bounds" in r.stdout, r.stdout
    raw, pos, out = open(fout, "rb").read(), 0, []
    for c in cases:
        if c[0] == "member":
            btype, nbytes, nlit, nmatch, matched, oob, hlit, hdist = struct.unpack_from("<8i", raw, pos)
            pos += 32
            ll, dl, cl = raw[pos:pos + 288], raw[pos + 288:pos + 320], raw[pos + 320:pos + 339]
            pos += 339
            g = dict(btype=btype, stream=raw[pos:pos + nbytes], literals=nlit, matches=nmatch, matched=matched, oob=oob,
                     hlit=hlit, hdist=hdist, ll=ll, dl=dl, cl=cl)
            pos += nbytes
            if histograms:
                h = struct.unpack_from("<316I", raw, pos)
                pos += 4 * 316
                g.update(ll_freq=list(h[:286]), d_freq=list(h[286:]))
            out.append(g)
        else:
            out.append(raw[pos:pos + len(c[2])])
            pos += len(c[2])
    assert pos == len(raw)
    return out


def all_inputs():
    """[(name, text)] of everything the fixture covers: the directed inputs, the model's own, the golden renderings, the fuzz
    members.  A text longer than a member is several members of one name."""
    return (list(B.named_inputs()) + list(B.model_inputs()) + list(zip(GOLDEN_NAMES, B.golden_renderings()))
            + [("fuzz%d" % k, B.fuzz_member(k)) for k in range(20)])


def entry(text, g):
    return dict(n=len(text), btype=g["btype"], bytes=len(g["stream"]), sha256=hashlib.sha256(g["stream"]).hexdigest(),
                literals=g["literals"], matches=g["matches"], matched=g["matched"])


def compute(exe, tmp, inputs, histograms=False):
    """-> ({name: [entry per member]}, {name: [the model's dict per member]})"""
    cases = [(name, m) for name, text in inputs for m in B.members(text)]
    got = run(exe, tmp, [("member", m) for _, m in cases], histograms)
    entries, raw = {name: [] for name, _ in inputs}, {name: [] for name, _ in inputs}
    for (name, m), g in zip(cases, got):
        entries[name].append(entry(m, g))
        raw[name].append(g)
    return entries, raw


def dumps(entries):
    """The fixture's text: one line per member, names in the order of all_inputs()."""
    lines = []
    for name, ms in entries.items():
        rows = ",\n".join("    " + json.dumps({k: e[k] for k in KEYS}) for e in ms)
        lines.append("  %s: [\n%s\n  ]" % (json.dumps(name), rows) if ms else "  %s: []" % json.dumps(name))
    return "{\n" + ",\n".join(lines) + "\n}\n"


def load():
    with open(FIXTURE) as f:
        return json.load(f)
