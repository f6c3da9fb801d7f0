#!/usr/bin/env python3
"""Formatting output records on the device against the host's formatter, for text that is already in host memory.

  (a) fastio.format_parallel on 16 threads (mio_format);
  (b) Engine.format_text, uploaded form: text and index go up, the formatted text comes back;
  (c) Engine.format_text, resident form, behind an Engine.filter_fastq call made outside the timed span;
  (d) fastio.format_parallel + Engine.bgzf_compress: the host's text uploaded again to be compressed;
  (e) Engine.format_text, resident form with bgzf=True: only BGZF members come back;
  and the three kernels alone, from the context's own events (rounds of their own).

Input: the text of tests/golden/test1.fastq.gz (1,000 reads of 251 bases) tiled to `--mib` MiB (default 256), selection = every
record, fastq and qual kinds.  One untimed round, then `--rounds` interleaved rounds of the arms timed by the wall clock around the
synchronous calls; median, minimum, maximum and interquartile range per arm.  The arms' results are compared once: (b) and (c)
with (a) byte for byte, (e) with (d).  Then one pair of CLI runs at -p 16 (FASTQ in, -o fastq -oc gz, -c false, --device_pack
--device_index --device_compress with and without --device_format), each in a process of its own.  Results: one JSON file
(profiles/device_format_rate.json); nothing here is a threshold, and no rate is promised.
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
from concurrent.futures import ThreadPoolExecutor

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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_format_rate.json"))
args = ap.parse_args()

golden = gzip.open(os.path.join(ROOT, "tests", "golden", "test1.fastq.gz")).read()
size = args.mib << 20
text = (golden * (size // len(golden) + 1))[:size]
text = text[:text.rfind(b"\n@") + 1]                         # whole records: the CLI pair reads the same bytes
reads = text.count(b"\n") // 4
idx = F.index(text, True, reads + 16, threads=args.threads)[0].copy()
assert len(idx) == reads
sel = np.arange(reads, dtype=np.int64)
KINDS = {"fastq": F.FMT_FASTQ, "qual": F.FMT_QUAL}


def spread(v):
    q = statistics.quantiles(v, n=4)
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "iqr": q[2] - q[0]}


def verdict(sp, host, device):
    both = sp[host]["iqr"] + sp[device]["iqr"]
    return {"device_faster_by_more_than_both_iqr": bool(sp[host]["median"] - sp[device]["median"] > both),
            "host_faster_by_more_than_both_iqr": bool(sp[device]["median"] - sp[host]["median"] > both)}


result = {"text_bytes": len(text), "reads": reads, "rounds": args.rounds, "host_threads": args.threads, "kinds": {}}
pool = ThreadPoolExecutor(args.threads)
with Engine(0) as eng:
    # the host formatter's pieces as the CLI takes them: written one by one, never joined (joined here for comparisons and for
    # the one upload of arm (d) only)
    pieces = lambda kind: F.format_parallel(pool, args.threads, text, idx, sel, kind)
    host = lambda kind: b"".join(bytes(p) for p in pieces(kind))
    for name, kind in KINDS.items():
        gen = [0]

        def resident(kind=kind, **kw):
            # the filter call that leaves text and index on the device is made outside the timed span
            r = eng.filter_fastq(text, True, reads + 16)
            gen[0] = r.resident
            return lambda: eng.format_text(idx=idx, kind=kind, resident=gen[0], **kw)
        arms = {
            "a_host_format": lambda kind=kind: pieces(kind),
            "b_device_uploaded": lambda kind=kind: eng.format_text(text, idx, kind=kind),
            "c_device_resident": None,
            "d_host_format_device_compress": lambda kind=kind: eng.bgzf_compress(host(kind)),
            "e_device_resident_compressed": None,
        }

        def run(arm):
            """-> (the result, milliseconds of the timed span)."""
            fn = arms[arm] or resident(bgzf=arm.startswith("e_"))
            t = time.perf_counter()
            out = fn()
            return out, (time.perf_counter() - t) * 1e3
        first = {arm: run(arm)[0] for arm in arms}           # untimed: pages are touched, buffers grow
        first["a_host_format"] = host(kind)
        assert first["b_device_uploaded"] == first["a_host_format"] == first["c_device_resident"]
        assert bytes(first["e_device_resident_compressed"]) == first["d_host_format_device_compress"]
        out_bytes = len(first["a_host_format"])
        del first
        ms = {arm: [] for arm in arms}
        for _ in range(args.rounds):
            for arm in arms:
                ms[arm].append(run(arm)[1])
        eng.timing(True)
        eng.timing_reset()
        for _ in range(3):
            eng.format_text(text, idx, kind=kind)
        kernel_ms = round(eng.kernel_times()["pack_text"][0] / 3.0, 3)
        eng.timing(False)
        sp = {arm: spread(v) for arm, v in ms.items()}
        result["kinds"][name] = {
            "formatted_bytes": out_bytes, "ms": ms, "ms_per_call": sp,
            "formatted_mb_per_second": {arm: out_bytes / 1e6 / (v["median"] * 1e-3) for arm, v in sp.items()},
            "uploaded_against_host": verdict(sp, "a_host_format", "b_device_uploaded"),
            "resident_against_host": verdict(sp, "a_host_format", "c_device_resident"),
            "resident_compressed_against_host_format_device_compress": verdict(sp, "d_host_format_device_compress", "e_device_resident_compressed"),
            "format_kernels_ms_per_call": kernel_ms}
pool.shutdown()

if not args.no_cli:
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "tiled.fastq")
        with open(path, "wb") as fh:
            fh.write(text)
        runs = {}
        for label, extra in (("host", []), ("device", ["--device_format"])):
            cmd = [sys.executable, os.path.join(ROOT, "moira.py"), "-ffq", path, "-op", os.path.join(td, label), "--silent", "-c", "false",
                   "-o", "fastq", "-oc", "gz", "-p", str(args.threads), "--device_pack", "--device_index", "--device_compress"] + extra
            t = time.perf_counter()
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
            sec = time.perf_counter() - t
            files = sorted(f for f in os.listdir(td) if f.startswith(label + "."))
            runs[label] = {"returncode": r.returncode, "seconds": sec, "reads_per_second": reads / sec,
                           "output_bytes": sum(os.path.getsize(os.path.join(td, f)) for f in files),
                           "files": [f.split(".", 1)[1] for f in files],
                           "messages": [l for l in r.stdout.splitlines() if "--device_" in l]}
        same = runs["host"]["files"] == runs["device"]["files"] and all(
            gzip.open(os.path.join(td, "host." + f)).read() == gzip.open(os.path.join(td, "device." + f)).read() for f in runs["host"]["files"])
        result["cli_pair"] = {
            "command": "moira.py -ffq tiled.fastq -c false -o fastq -oc gz -p %d --device_pack --device_index --device_compress [--device_format]" % args.threads,
            "input_bytes": len(text), "reads": reads, "runs": runs, "outputs_equal_after_decompression": bool(same)}

result["note"] = ("arms (a), (b), (d) start from text that lies in host memory; (c) and (e) from what a filter_fastq call outside the timed "
                  "span left on the device; every arm ends with its output in host memory; measured once, no rate is promised")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(result, fh, indent=1)
print(json.dumps({k: {a: v[a] for a in ("ms_per_call", "format_kernels_ms_per_call", "uploaded_against_host", "resident_against_host",
                                        "resident_compressed_against_host_format_device_compress")} for k, v in result["kinds"].items()}))
if "cli_pair" in result:
    print(json.dumps(result["cli_pair"]))
