#!/usr/bin/env python3
"""Indexing FASTQ records on the device against the host's indexer, for text that is already in host memory.

  (a) the index alone:   libmoira_io's mio_fastq_index_mt on 16 threads (fastio.index) against Engine.fastq_index
                         (mpb_fastq_index_host: upload, k_fq_lines / _scan / _starts / _rows, the rows copied back);
  (b) index and filter:  fastio.index + Engine.filter_text against Engine.filter_fastq (one upload, the index on the device);
  (c) the four kernels alone, from the context's own events (rounds of their own).

Input: the text of tests/golden/test1.fastq.gz (1,000 reads of 251 bases) tiled to `--mib` MiB (default 256).  One untimed round,
then `--rounds` interleaved rounds of the arms timed by the wall clock around the synchronous calls; median, minimum, maximum and
interquartile range per arm.  The device's index is compared with the host's once.  Then one pair of CLI runs at -p 16 and one at
-p 1 (FASTQ in, FASTQ out, -c false, --device_pack with and without --device_index), each in a process of its own.  Results: one
JSON file (profiles/device_index_rate.json); nothing here is a threshold, and no rate is promised.
"""
import argparse
import gzip
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
from moira_amd import fastio as F  # noqa: E402
from moira_amd.engine import Engine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--mib", type=int, default=256)
ap.add_argument("--rounds", type=int, default=20)
ap.add_argument("--threads", type=int, default=16)
ap.add_argument("--no_cli", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_index_rate.json"))
args = ap.parse_args()

golden = gzip.open(os.path.join(ROOT, "tests", "golden", "test1.fastq.gz")).read()
size = args.mib << 20
text = (golden * (size // len(golden) + 1))[:size]
text = text[:text.rfind(b"\n@") + 1]                         # whole records: the CLI pairs read the same bytes
reads = text.count(b"\n") // 4
cap = reads + 16


def spread(v):
    q = statistics.quantiles(v, n=4)
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "iqr": q[2] - q[0]}


def verdict(sp, host, device):
    both = sp[host]["iqr"] + sp[device]["iqr"]
    return {"device_faster_by_more_than_both_iqr": bool(sp[host]["median"] - sp[device]["median"] > both),
            "host_faster_by_more_than_both_iqr": bool(sp[device]["median"] - sp[host]["median"] > both)}


result = {"text_bytes": len(text), "reads": reads, "rounds": args.rounds, "host_threads": args.threads}
with Engine(0) as eng:
    arms = {
        "host_index": lambda: F.index(text, True, cap, threads=args.threads),
        "device_index": lambda: eng.fastq_index(text, True, cap),
        "host_index_filter": lambda: eng.filter_text(text, F.index(text, True, cap, threads=args.threads)[0]),
        "device_index_filter": lambda: eng.filter_fastq(text, True, cap),
    }
    first = {k: fn() for k, fn in arms.items()}              # untimed: pages are touched, buffers grow
    hidx, hcons, hbad = first["host_index"]
    didx, dcons, dbad = first["device_index"]
    assert len(hidx) == reads and hbad is None and dbad is None and hcons == dcons == len(text) and np.array_equal(hidx, didx)
    hf, df = first["host_index_filter"], first["device_index_filter"]
    assert np.array_equal(df.idx, hidx) and np.array_equal(hf.ee.view(np.uint64), df.ee.view(np.uint64)) and np.array_equal(hf.passed, df.passed)
    del first, hf, df
    ms = {k: [] for k in arms}
    for _ in range(args.rounds):
        for arm, fn in arms.items():
            t = time.perf_counter()
            fn()
            ms[arm].append((time.perf_counter() - t) * 1e3)
    eng.timing(True)
    eng.timing_reset()
    for _ in range(3):
        eng.fastq_index(text, True, cap)
    kernel_ms = {k: round(v[0] / 3.0, 3) for k, v in sorted(eng.kernel_times().items()) if v[1] and k.startswith("fq_")}
    eng.timing(False)
    sp = {k: spread(v) for k, v in ms.items()}
    result.update({
        "ms": ms, "ms_per_call": sp,
        "text_mb_per_second": {k: len(text) / 1e6 / (v["median"] * 1e-3) for k, v in sp.items()},
        "index_alone": verdict(sp, "host_index", "device_index"),
        "index_and_filter": verdict(sp, "host_index_filter", "device_index_filter"),
        "kernel_ms_per_call": kernel_ms,
        "kernel_text_mb_per_second": len(text) / 1e6 / (sum(kernel_ms.values()) * 1e-3) if kernel_ms else None})

if not args.no_cli:
    # one pair of CLI runs per thread count, a process each: seconds of the whole run
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "tiled.fastq")
        with open(path, "wb") as fh:
            fh.write(text)
        result["cli_pairs"] = {}
        for p in (args.threads, 1):
            runs = {}
            for label, extra in (("host", []), ("device", ["--device_index"])):
                prefix = "%s%d" % (label, p)
                cmd = [sys.executable, os.path.join(ROOT, "moira.py"), "-ffq", path, "-op", os.path.join(td, prefix), "--silent", "-c", "false",
                       "-o", "fastq", "-p", str(p), "--device_pack"] + extra
                t = time.perf_counter()
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
                sec = time.perf_counter() - t
                files = sorted(f for f in os.listdir(td) if f.startswith(prefix + "."))
                runs[label] = {"returncode": r.returncode, "seconds": sec, "reads_per_second": reads / sec,
                               "output_bytes": sum(os.path.getsize(os.path.join(td, f)) for f in files),
                               "files": [f.split(".", 1)[1] for f in files],
                               "messages": [l for l in r.stdout.splitlines() if "--device_index" in l]}
            same = runs["host"]["files"] == runs["device"]["files"] and all(
                open(os.path.join(td, "host%d.%s" % (p, f)), "rb").read() == open(os.path.join(td, "device%d.%s" % (p, f)), "rb").read()
                for f in runs["host"]["files"])
            result["cli_pairs"]["p%d" % p] = {
                "command": "moira.py -ffq tiled.fastq -c false -o fastq -p %d --device_pack [--device_index]" % p,
                "input_bytes": len(text), "reads": reads, "runs": runs, "outputs_equal": bool(same)}
            for f in os.listdir(td):
                if f != "tiled.fastq":
                    os.remove(os.path.join(td, f))

result["note"] = ("every arm starts from text that lies in host memory and ends with the index (and the results) in host memory; the "
                  "device arms include the upload and the copies back; measured once, no rate is promised")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(result, fh, indent=1)
print(json.dumps({k: result[k] for k in ("ms_per_call", "text_mb_per_second", "index_alone", "index_and_filter", "kernel_ms_per_call",
                                         "kernel_text_mb_per_second")}))
if "cli_pairs" in result:
    print(json.dumps(result["cli_pairs"]))
