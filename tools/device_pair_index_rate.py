#!/usr/bin/env python3
"""Paired FASTQ from text alone against the host's indexes, for one chunk of pairs whose two texts lie in host memory.

  (a) host_index:   fastio.index x 2 (`--threads` threads each, one after the other), fastio.first_header_mismatch, then
      Engine.contigs_filter_text (which builds mpb_pair_rows, the size classes and the lists on the host and uploads them);
  (b) device_index: Engine.contigs_filter_fastq (mpb_contigs_filter_fastq_host: both indexes, the header comparison, the
      descriptors, classes and lists on the device; each text goes up once).

Input: the golden paired inputs (tests/golden/test1.fastq.gz + test2.fastq.bz2, 1,000 pairs of 2 x 251), tiled; both arms take
the first cli.PAIR_CHUNK_READS pairs (max_records).  Both arms are synchronous calls timed by the wall clock, interleaved,
`--rounds` rounds after one untimed round.  Reported: ms per chunk of every round, median, minimum, maximum and interquartile
range per arm, equality of the two arms' results, the verdict by the README's rule (a difference counts when it is larger than
the two interquartile ranges together), arm (a)'s time by its parts, and -- from rounds of their own with the context's own
timing on -- the kernels' times per chunk (the four pairing kernels run inside contig_rows' span).  Then one pair of whole CLI
runs (paired FASTQ, -p `--threads`, --device_contigs --device_pack, with and without --device_pair_index), a process each.
Results: one JSON file (profiles/device_pair_index_rate.json); nothing here is a threshold, and no rate is promised.
"""
import argparse
import bz2
import gzip
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from moira_amd import cli  # noqa: E402
from moira_amd import fastio as F  # noqa: E402
from moira_amd.engine import Engine  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=cli.PAIR_CHUNK_READS)
ap.add_argument("--rounds", type=int, default=20)
ap.add_argument("--threads", type=int, default=16)
ap.add_argument("--no_cli", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_pair_index_rate.json"))
args = ap.parse_args()

gold = gzip.open(os.path.join(GOLD, "test1.fastq.gz")).read(), bz2.open(os.path.join(GOLD, "test2.fastq.bz2")).read()
m = len(F.index(gold[0], True, 1 << 20)[0])
n = args.pairs
reps = (n + m - 1) // m
ftext, rtext = gold[0] * reps, gold[1] * reps


def spread(v):
    q = statistics.quantiles(v, n=4)
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "iqr": q[2] - q[0]}


result = {"pairs": n, "golden_pairs": m, "rounds": args.rounds, "host_threads": args.threads, "text_bytes": len(ftext) + len(rtext),
          "host_index": [], "device_index": []}
with Engine(0) as eng:
    parts = {"index_x2": [], "first_header_mismatch": [], "contigs_filter_text": []}

    def host_index():
        t0 = time.perf_counter()
        fi, ri = F.index(ftext, True, n, threads=args.threads)[0], F.index(rtext, True, n, threads=args.threads)[0]
        t1 = time.perf_counter()
        bad = F.first_header_mismatch(ftext, fi, rtext, ri)
        t2 = time.perf_counter()
        r = eng.contigs_filter_text(ftext, fi, rtext, ri, 33)
        t3 = time.perf_counter()
        for k, v in zip(parts, (t1 - t0, t2 - t1, t3 - t2)):
            parts[k].append(v * 1e3)
        return fi, ri, bad, r

    def device_index():
        return eng.contigs_filter_fastq(ftext, rtext, max_records=n)

    (fi, ri, bad, r), g = host_index(), device_index()           # untimed: buffers grow, pages are touched
    built = np.nonzero(r.done)[0]
    same = [np.array_equal(np.asarray(getattr(g, k))[built].view(np.uint8), np.asarray(getattr(r, k))[built].view(np.uint8))
            for k in ("ee", "ns", "passed", "lens", "has_n", "cidx", "aux")]
    result["rec_cap"], result["handed_back"], result["calls_of_the_entry"] = int(g.rec_cap), int(g.n_handed_back), int(g.calls)
    result["results_equal"] = bool(all(same) and np.array_equal(g.fidx, fi) and np.array_equal(g.ridx, ri) and g.mismatch == bad == -1 and
                                   np.array_equal(g.done, r.done) and np.array_equal(g.filtered, r.filtered) and g.rec_cap == r.rec_cap and
                                   g.n_pass == r.n_pass and g.filter_error is None and r.filter_error is None)
    assert result["results_equal"], same
    for v in parts.values():
        del v[:]
    for _ in range(args.rounds):
        for name, fn in (("host_index", host_index), ("device_index", device_index)):
            t = time.perf_counter()
            fn()
            result[name].append((time.perf_counter() - t) * 1e3)
    result["host_index_parts_median_ms"] = {k: statistics.median(v) for k, v in parts.items()}
    # the kernels alone, from the context's own events (rounds of their own: the events cost the timed rounds nothing)
    eng.timing(True)
    kernel_ms = {}
    for name, fn in (("host_index", host_index), ("device_index", device_index)):
        eng.timing_reset()
        for _ in range(3):
            fn()
        kernel_ms[name] = {k: round(v[0] / 3.0, 4) for k, v in sorted(eng.kernel_times().items()) if v[1]}
    eng.timing(False)
    result["kernel_ms_per_chunk"] = kernel_ms

sp = result["ms_per_chunk"] = {k: spread(result[k]) for k in ("host_index", "device_index")}
both = sp["host_index"]["iqr"] + sp["device_index"]["iqr"]
result["verdict"] = {"device_faster_by_more_than_both_iqr": bool(sp["host_index"]["median"] - sp["device_index"]["median"] > both),
                     "host_faster_by_more_than_both_iqr": bool(sp["device_index"]["median"] - sp["host_index"]["median"] > both)}
result["pairs_per_second"] = {k: n / (v["median"] * 1e-3) for k, v in sp.items()}

if not args.no_cli:
    # one pair of whole CLI runs, a process each: seconds of the run, outputs compared
    with tempfile.TemporaryDirectory() as td:
        names = [os.path.join(td, "tiled%d.fastq" % k) for k in (1, 2)]
        for name, text in zip(names, (ftext, rtext)):
            with open(name, "wb") as fh:
                fh.write(text)
        runs = {}
        for label, extra in (("host", []), ("device", ["--device_pair_index"])):
            cmd = [sys.executable, os.path.join(ROOT, "moira.py"), "-ffq", names[0], "-rfq", names[1], "--paired", "-op", os.path.join(td, label),
                   "--silent", "-c", "false", "-o", "fastq", "-p", str(args.threads), "--device_contigs", "--device_pack"] + extra
            t = time.perf_counter()
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
            sec = time.perf_counter() - t
            files = sorted(f for f in os.listdir(td) if f.startswith(label + "."))
            runs[label] = {"returncode": p.returncode, "seconds": sec, "pairs_per_second": m * reps / sec,
                           "files": [f.split(".", 1)[1] for f in files],
                           "messages": [l for l in p.stdout.splitlines() if "--device_pair_index" in l]}
        equal = runs["host"]["files"] == runs["device"]["files"] and all(
            open(os.path.join(td, "host." + f), "rb").read() == open(os.path.join(td, "device." + f), "rb").read() for f in runs["host"]["files"])
        result["cli_pair"] = {"command": "moira.py -ffq tiled1.fastq -rfq tiled2.fastq --paired -c false -o fastq -p %d --device_contigs "
                                         "--device_pack [--device_pair_index]" % args.threads,
                              "pairs": m * reps, "runs": runs, "outputs_equal": bool(equal)}

result["note"] = ("both arms start from the two texts in host memory and end with contigs, verdicts and both indexes in host memory; uploads "
                  "and copies back included; handed-back pairs are NOT rebuilt in either arm's time; measured once, no rate is promised")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(result, fh, indent=1)
print(json.dumps({k: result[k] for k in ("ms_per_chunk", "verdict", "host_index_parts_median_ms", "pairs_per_second", "handed_back",
                                         "calls_of_the_entry", "results_equal", "kernel_ms_per_chunk")}))
if "cli_pair" in result:
    print(json.dumps(result["cli_pair"]))
