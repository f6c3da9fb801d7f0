#!/usr/bin/env python3
"""Parsing, packing and filtering a chunk of fasta+qual text on the device against the host parser with the device text filter,
for one chunk of the CLI.

  (a) fastio.fasta_qual_index (mio_fasta_qual_index: one thread, every quality from its decimal text) + Engine.filter_text on
      what it built (fastq_offset 0); the two parts are also given apart;
  (b) Engine.filter_fasta_qual: both texts go up once; line tables, slots, index, pack and filter on the device;
  and the kernels of (b) alone, from the context's own events (a round of its own).

Input: the reads of tests/golden/test1.fastq.gz rendered to fasta+qual by tests/golden_io.py:write_fasta_qual and tiled to
`--mib` MiB of qual text (default 256) in host memory.  write_fasta_qual gives every 37th read a score of 300, which the
byte-level path declines on either side; those reads are left out of the timed text, and ONE untimed call of each arm on the
text that holds them records what becomes of it (the device hands it back, the host function says unsupported: the line parser's).
One untimed round, then `--rounds` interleaved rounds of the arms timed by the wall clock around the synchronous calls; median,
minimum, maximum and interquartile range per arm; the arms' results are compared in every round.  Then one pair of CLI runs at
-p 16 on the same two files (-c true, with and without --device_fasta_qual), each in a process of its own.  Results: one JSON
file (profiles/device_fasta_qual_rate.json); an arm wins only when it is faster by more than the two interquartile ranges
together; nothing here is a threshold, and no rate is promised.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import golden_io as G  # noqa: E402
from moira_amd import fastio as F  # noqa: E402
from moira_amd.engine import Engine, NotTaken  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--mib", type=int, default=256)
ap.add_argument("--rounds", type=int, default=20)
ap.add_argument("--threads", type=int, default=16)
ap.add_argument("--no_cli", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_fasta_qual_rate.json"))
args = ap.parse_args()


def rendered(keep):
    """write_fasta_qual's two texts of the golden reads `keep` selects (by position) -> (fasta, qual) bytes."""
    recs = G.read_fastq_records(os.path.join(ROOT, "tests", "golden", "test1.fastq.gz"))
    with tempfile.TemporaryDirectory() as td:
        fa, qu = os.path.join(td, "g.fasta"), os.path.join(td, "g.qual")
        G.write_fasta_qual(fa, qu, recs)
        f, q = open(fa, "rb").read().split(b"\n"), open(qu, "rb").read().split(b"\n")
    pick = [i for i in range(len(recs)) if keep(i)]
    return (b"".join(f[2 * i] + b"\n" + f[2 * i + 1] + b"\n" for i in pick), b"".join(q[2 * i] + b"\n" + q[2 * i + 1] + b"\n" for i in pick),
            len(pick))


def spread(v):
    q = statistics.quantiles(v, n=4)
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "iqr": q[2] - q[0]}


def verdict(sp, host, device):
    both = sp[host]["iqr"] + sp[device]["iqr"]
    faster, slower = sp[host]["median"] - sp[device]["median"] > both, sp[device]["median"] - sp[host]["median"] > both
    says = ("the device call is faster than the host parser plus the text filter by more than the two interquartile ranges together" if faster
            else "the host parser plus the text filter is faster than the device call by more than the two interquartile ranges together"
            if slower else "no difference beyond the two interquartile ranges together")
    return {"device_faster_by_more_than_both_iqr": bool(faster), "host_faster_by_more_than_both_iqr": bool(slower), "says": says}


f1, q1, per_tile = rendered(lambda i: i % 37 != 5)
tiles = max(1, (args.mib << 20) // len(q1))
ftext, qtext, reads = f1 * tiles, q1 * tiles, per_tile * tiles
out, idx = np.empty(2 * len(ftext) + 16, np.uint8), np.empty((reads + 16, F.IDX_COLS), np.int64)
result = {"fasta_bytes": len(ftext), "qual_bytes": len(qtext), "reads": reads, "reads_left_out_per_1000": 1000 - per_tile,
          "rounds": args.rounds, "host_threads": args.threads}

with Engine(0) as eng:
    def host():
        t0 = time.perf_counter()
        n, fc, qc, used = F.fasta_qual_index(ftext, qtext, True, reads + 16, out, idx)
        t1 = time.perf_counter()
        r = eng.filter_text(out[:used], idx[:n], fastq_offset=0)
        t2 = time.perf_counter()
        return (out[:used], idx[:n], fc, qc, r), {"a_host_parse_then_filter_text": (t2 - t0) * 1e3, "a1_host_parse": (t1 - t0) * 1e3,
                                                 "a2_filter_text": (t2 - t1) * 1e3}

    def device():
        t0 = time.perf_counter()
        r = eng.filter_fasta_qual(ftext, qtext, True, reads + 16)
        return (r.text, r.idx, r.f_consumed, r.q_consumed, r), {"b_filter_fasta_qual": (time.perf_counter() - t0) * 1e3}

    def same(a, b):
        return bool(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2:4] == b[2:4] and
                    np.array_equal(a[4].ee.view(np.uint64), b[4].ee.view(np.uint64)) and np.array_equal(a[4].ns, b[4].ns) and
                    np.array_equal(a[4].passed, b[4].passed) and np.array_equal(a[4].has_n, b[4].has_n))
    a, b = host()[0], device()[0]                            # untimed: pages are touched, buffers grow
    assert len(a[1]) == reads and same(a, b)
    ms, equal, handed_back = {}, 0, 0
    for _ in range(args.rounds):
        got = {}
        for arm in (host, device):
            try:
                got[arm.__name__], took = arm()
            except NotTaken:
                handed_back += 1
                continue
            for k, v in took.items():
                ms.setdefault(k, []).append(v)
        equal += int(len(got) == 2 and same(got["host"], got["device"]))
    eng.timing(True)
    eng.timing_reset()
    eng.filter_fasta_qual(ftext, qtext, True, reads + 16)
    kernels = {name: {"ms": round(t, 3), "spans": n} for name, (t, n) in eng.kernel_times().items() if n}
    eng.timing(False)
    # the text as write_fasta_qual leaves it, scores of 300 included: what becomes of it on either side
    fd, qd, _ = rendered(lambda i: True)
    try:
        eng.filter_fasta_qual(fd, qd)
        dev = "taken"
    except NotTaken as e:
        dev = {"why": str(e), "which": e.which, "bad_record": e.bad_record}
    try:
        F.fasta_qual_index(fd, qd, True, 2000, out, idx)
        hst = "taken"
    except F.Unsupported as e:
        hst = "unsupported: %s" % e
    sp = {arm: spread(v) for arm, v in ms.items()}
    result.update({"ms": ms, "ms_per_call": sp, "reads_per_second": {arm: reads / (v["median"] * 1e-3) for arm, v in sp.items()},
                   "qual_mib_per_second": {arm: len(qtext) / 2 ** 20 / (v["median"] * 1e-3) for arm, v in sp.items()},
                   "rounds_with_equal_results": equal, "calls_handed_back": handed_back,
                   "device_against_host": verdict(sp, "a_host_parse_then_filter_text", "b_filter_fasta_qual"),
                   "kernels_of_one_device_call": kernels, "with_the_scores_of_300": {"device": dev, "host": hst}})

if not args.no_cli:
    with tempfile.TemporaryDirectory() as td:
        fa, qu = os.path.join(td, "tiled.fasta"), os.path.join(td, "tiled.qual")
        with open(fa, "wb") as fh:
            fh.write(ftext)
        with open(qu, "wb") as fh:
            fh.write(qtext)
        runs = {}
        for label, extra in (("host", []), ("device", ["--device_fasta_qual"])):
            cmd = [sys.executable, os.path.join(ROOT, "moira.py"), "-ff", fa, "-fq", qu, "-op", os.path.join(td, label), "--silent",
                   "-p", str(args.threads)] + extra
            t = time.perf_counter()
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
            sec = time.perf_counter() - t
            files = sorted(f for f in os.listdir(td) if f.startswith(label + "."))
            runs[label] = {"returncode": r.returncode, "seconds": sec, "reads_per_second": reads / sec,
                           "output_bytes": sum(os.path.getsize(os.path.join(td, f)) for f in files),
                           "files": [f.split(".", 1)[1] for f in files],
                           "messages": [l for l in r.stdout.splitlines() if "--device_" in l]}
        same_files = runs["host"]["files"] == runs["device"]["files"] and all(
            open(os.path.join(td, "host." + f), "rb").read() == open(os.path.join(td, "device." + f), "rb").read() for f in runs["host"]["files"])
        result["cli_pair"] = {"command": "moira.py -ff tiled.fasta -fq tiled.qual -p %d [--device_fasta_qual]" % args.threads,
                              "reads": reads, "runs": runs, "outputs_equal": bool(same_files)}

result["note"] = ("both arms start from the two texts in host memory and end with slots, index and filter results in host memory; arm (a) "
                  "parses on one host thread, as the CLI does today; in a CLI run either parser works beside the writers; measured once, "
                  "no rate is promised")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(result, fh, indent=1)
print(json.dumps({k: result[k] for k in ("reads", "qual_bytes", "ms_per_call", "qual_mib_per_second", "rounds_with_equal_results",
                                          "calls_handed_back", "device_against_host", "kernels_of_one_device_call", "with_the_scores_of_300")}))
if "cli_pair" in result:
    print(json.dumps(result["cli_pair"]))
