#!/usr/bin/env python3
"""Compressing .gz output on the device against the host's zlib, for text that is already in host memory.

  (i)  host:   cli.bgzf_compress (zlib level 4) over 1 MiB blocks on a pool of 16 threads, as _BlockCompressedWriter uses it;
  (ii) device: Engine.bgzf_compress (mpb_bgzf_compress_host: upload, k_bgzf_deflate, k_bgzf_scan, k_bgzf_frame, copy-back inside
       the call; the CRC-32 of every member on the host meanwhile).

Input: the text of tests/golden/test1.fastq.gz (1,000 reads of 251 bases) tiled to `--mib` MiB (default 256), and the fasta and
qual renderings of the same reads tiled to the same size.  Per text: one untimed round, then `--rounds` interleaved rounds of both
arms timed by the wall clock; median, minimum, maximum and interquartile range per arm; compressed bytes / text bytes of both
arms; the three kernels alone from the context's own events (a round of its own).  The device's output is inflated with zlib and
compared with the text once per text.  Then one pair of CLI runs on the tiled FASTQ text (-o fastq -oc gz -c false, with and
without --device_compress), each in a process of its own.  Results: one JSON file (profiles/device_bgzf_rate.json); nothing here
is a threshold, and no rate is promised.
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from moira_amd import cli  # noqa: E402
from moira_amd.engine import Engine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--mib", type=int, default=256)
ap.add_argument("--rounds", type=int, default=20)
ap.add_argument("--threads", type=int, default=16)
ap.add_argument("--no_cli", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_bgzf_rate.json"))
args = ap.parse_args()

golden = gzip.open(os.path.join(ROOT, "tests", "golden", "test1.fastq.gz")).read()
lines = golden.split(b"\n")
fasta, qual = [], []
for k in range(0, len(lines) - 3, 4):
    h, s, q = lines[k][1:], lines[k + 1], lines[k + 3]
    fasta.append(b">" + h + b"\n" + s + b"\n")
    qual.append(b">" + h + b"\n" + b" ".join(b"%d" % (c - 33) for c in q) + b"\n")
size = args.mib << 20


def tiled(text):
    return (text * (size // len(text) + 1))[:size]


texts = {"fastq": tiled(golden), "fasta": tiled(b"".join(fasta)), "qual": tiled(b"".join(qual))}
BLOCK = cli._BlockCompressedWriter.BLOCK
pool = ThreadPoolExecutor(args.threads)


def spread(v):
    q = statistics.quantiles(v, n=4)
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "iqr": q[2] - q[0]}


result = {"text_mib": args.mib, "rounds": args.rounds, "host_threads": args.threads, "host_level": 4, "texts": {}}
with Engine(0) as eng:
    for name, text in texts.items():
        mv = memoryview(text)

        def host():
            return sum(len(z) for z in pool.map(lambda k: cli.bgzf_compress(mv[k:k + BLOCK], 4), range(0, len(text), BLOCK)))

        def device():
            return len(eng.bgzf_compress(text))

        host_bytes = host()                                              # untimed: pages are touched, buffers grow
        out = eng.bgzf_compress(text)
        assert gzip.decompress(out + cli.BGZF_EOF) == text
        stats = eng.bgzf_stats()
        ms = {"host": [], "device": []}
        for _ in range(args.rounds):
            for arm, fn in (("host", host), ("device", device)):
                t = time.perf_counter()
                fn()
                ms[arm].append((time.perf_counter() - t) * 1e3)
        eng.timing(True)
        eng.timing_reset()
        for _ in range(3):
            device()
        kernel_ms = {k: round(v[0] / 3.0, 3) for k, v in sorted(eng.kernel_times().items()) if v[1]}
        eng.timing(False)
        sp = {k: spread(v) for k, v in ms.items()}
        result["texts"][name] = {
            "text_bytes": len(text), "ms": ms, "ms_per_call": sp,
            "mb_per_second": {k: len(text) / 1e6 / (v["median"] * 1e-3) for k, v in sp.items()},
            "device_faster_by_more_than_both_iqr": bool(sp["host"]["median"] - sp["device"]["median"] > sp["host"]["iqr"] + sp["device"]["iqr"]),
            "compressed_bytes": {"host": host_bytes, "device": len(out)},
            "compressed_over_text": {"host": host_bytes / len(text), "device": len(out) / len(text)},
            "device_over_host_size": len(out) / host_bytes,
            "stats": stats, "kernel_ms_per_call": kernel_ms,
            "kernels_mb_per_second": len(text) / 1e6 / (sum(kernel_ms.values()) * 1e-3) if kernel_ms else None}
pool.shutdown()

if not args.no_cli:
    # one pair of CLI runs on the same FASTQ text, a process each: seconds of the whole run and the bytes of its outputs
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "tiled.fastq")
        with open(path, "wb") as fh:
            fh.write(texts["fastq"][:texts["fastq"].rfind(b"\n@") + 1])
        runs = {}
        for label, extra in (("host", []), ("device", ["--device_compress"])):
            cmd = [sys.executable, os.path.join(ROOT, "moira.py"), "-ffq", path, "-op", os.path.join(td, label), "--silent", "-c", "false",
                   "-o", "fastq", "-oc", "gz", "-p", str(args.threads)] + extra
            t = time.perf_counter()
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
            sec = time.perf_counter() - t
            files = sorted(f for f in os.listdir(td) if f.startswith(label + "."))
            runs[label] = {"returncode": p.returncode, "seconds": sec, "output_bytes": sum(os.path.getsize(os.path.join(td, f)) for f in files),
                           "files": [f.split(".", 1)[1] for f in files], "messages": [l for l in p.stdout.splitlines() if "--device_compress" in l]}
        same = all(gzip.open(os.path.join(td, "host." + f)).read() == gzip.open(os.path.join(td, "device." + f)).read() for f in runs["host"]["files"])
        result["cli_pair"] = {"command": "moira.py -ffq tiled.fastq -c false -o fastq -oc gz -p %d [--device_compress]" % args.threads,
                              "input_bytes": os.path.getsize(path), "runs": runs, "outputs_equal_after_decompression": bool(same)}

result["note"] = ("both arms compress text that lies in host memory; the device arm includes upload, the host's CRC-32 and the copy back; "
                  "measured once, no rate is promised")
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(result, fh, indent=1)
print(json.dumps({n: {k: t[k] for k in ("ms_per_call", "mb_per_second", "compressed_over_text", "device_over_host_size", "kernel_ms_per_call",
                                        "device_faster_by_more_than_both_iqr")} for n, t in result["texts"].items()}))
if "cli_pair" in result:
    print(json.dumps(result["cli_pair"]))
