#!/usr/bin/env python3
"""Inflating BGZF .gz input on the device against the host's inflater, for compressed bytes that are already in host memory.

  (i)  host:   libmoira_io's mio_bgzf_inflate_mt on 16 threads, as fastio.GzipReader uses it;
  (ii) device: Engine.bgzf_inflate (mpb_bgzf_inflate_host: the rows, upload, k_bgzf_inflate, copy-back of status and text, the
       CRC-32 of every member on the host -- all inside the call).

Input: the text of tests/golden/test1.fastq.gz (1,000 reads of 251 bases) tiled to `--mib` MiB (default 256), compressed once by
cli.bgzf_compress (zlib level 4) and once by Engine.bgzf_compress (the device's own members).  Per input: mio_bgzf_scan once, one
untimed round, then `--rounds` interleaved rounds of both arms timed by the wall clock around the synchronous calls; median,
minimum, maximum and interquartile range per arm; the kernel alone from the context's own events (a round of its own).  The
device's text is compared with the input text once per input.  Then one pair of CLI runs on the zlib-compressed input (BGZF in,
FASTQ out, -c false, with and without --device_inflate), each in a process of its own.  Results: one JSON file
(profiles/device_bgzf_inflate_rate.json); nothing here is a threshold, and no rate is promised.
"""
import argparse
import ctypes as C
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
from moira_amd import cli  # noqa: E402
from moira_amd import fastio as F  # noqa: E402
from moira_amd.engine import Engine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--mib", type=int, default=256)
ap.add_argument("--rounds", type=int, default=20)
ap.add_argument("--threads", type=int, default=16)
ap.add_argument("--no_cli", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_bgzf_inflate_rate.json"))
args = ap.parse_args()

golden = gzip.open(os.path.join(ROOT, "tests", "golden", "test1.fastq.gz")).read()
size = args.mib << 20
text = (golden * (size // len(golden) + 1))[:size]
text = text[:text.rfind(b"\n@") + 1]                         # whole records: the CLI pair reads the same bytes
BLOCK = 1 << 24
lib = F.load()


def spread(v):
    q = statistics.quantiles(v, n=4)
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "iqr": q[2] - q[0]}


result = {"text_bytes": len(text), "rounds": args.rounds, "host_threads": args.threads, "inputs": {}}
with Engine(0) as eng:
    with ThreadPoolExecutor(args.threads) as pool:
        mv = memoryview(text)
        zlib_blob = b"".join(pool.map(lambda k: cli.bgzf_compress(mv[k:k + BLOCK], 4), range(0, len(text), BLOCK)))
    blobs = {"zlib_level4": zlib_blob, "device_written": eng.bgzf_compress(text)}
    for name, blob in blobs.items():
        buf = np.frombuffer(blob + b"\0" * 8, np.uint8)
        cap = len(blob) // 26 + 1
        offs, sizes, out_offs, why = np.empty(cap, np.int64), np.empty(cap, np.int32), np.empty(cap + 1, np.int64), C.c_int32(0)
        nb = lib.mio_bgzf_scan(buf.ctypes.data, len(blob), cap, 1 << 40, offs.ctypes.data, sizes.ctypes.data, out_offs.ctypes.data,
                               C.addressof(why))
        assert nb > 0 and int(out_offs[nb]) == len(text) and int(offs[nb - 1]) + int(sizes[nb - 1]) == len(blob)
        offs, sizes, out_offs = offs[:nb].copy(), sizes[:nb].copy(), out_offs[:nb + 1].copy()
        out_h, out_d = np.empty(len(text), np.uint8), np.empty(len(text), np.uint8)

        def host():
            assert lib.mio_bgzf_inflate_mt(buf.ctypes.data, offs.ctypes.data, sizes.ctypes.data, out_offs.ctypes.data, nb,
                                           out_h.ctypes.data, args.threads) == 0

        def device():
            return eng.bgzf_inflate(buf[:len(blob)], offs, sizes, out_offs, out=out_d)

        host()                                               # untimed: pages are touched, buffers grow
        _, done, _ = device()
        stats = eng.bgzf_inflate_stats()
        assert out_h.tobytes() == text
        assert done.all() and out_d.tobytes() == text, stats
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
        result["inputs"][name] = {
            "compressed_bytes": len(blob), "members": int(nb), "ms": ms, "ms_per_call": sp,
            "text_mb_per_second": {k: len(text) / 1e6 / (v["median"] * 1e-3) for k, v in sp.items()},
            "device_faster_by_more_than_both_iqr": bool(sp["host"]["median"] - sp["device"]["median"] > sp["host"]["iqr"] + sp["device"]["iqr"]),
            "host_faster_by_more_than_both_iqr": bool(sp["device"]["median"] - sp["host"]["median"] > sp["host"]["iqr"] + sp["device"]["iqr"]),
            "stats": stats, "kernel_ms_per_call": kernel_ms,
            "kernel_text_mb_per_second": len(text) / 1e6 / (sum(kernel_ms.values()) * 1e-3) if kernel_ms else None}

if not args.no_cli:
    # one pair of CLI runs on the zlib-compressed input, a process each: seconds of the whole run
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "tiled.fastq.gz")
        with open(path, "wb") as fh:
            fh.write(zlib_blob + cli.BGZF_EOF)
        runs = {}
        for label, extra in (("host", []), ("device", ["--device_inflate"])):
            cmd = [sys.executable, os.path.join(ROOT, "moira.py"), "-ffq", path, "-op", os.path.join(td, label), "--silent", "-c", "false",
                   "-o", "fastq", "-p", str(args.threads)] + extra
            t = time.perf_counter()
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
            sec = time.perf_counter() - t
            files = sorted(f for f in os.listdir(td) if f.startswith(label + "."))
            runs[label] = {"returncode": p.returncode, "seconds": sec, "output_bytes": sum(os.path.getsize(os.path.join(td, f)) for f in files),
                           "files": [f.split(".", 1)[1] for f in files], "messages": [l for l in p.stdout.splitlines() if "--device_inflate" in l]}
        same = all(open(os.path.join(td, "host." + f), "rb").read() == open(os.path.join(td, "device." + f), "rb").read()
                   for f in runs["host"]["files"]) and runs["host"]["files"] == runs["device"]["files"]
        reads = text.count(b"\n") // 4
        for r in runs.values():
            r["reads_per_second"] = reads / r["seconds"]
        result["cli_pair"] = {"command": "moira.py -ffq tiled.fastq.gz -c false -o fastq -p %d [--device_inflate]" % args.threads,
                              "input_bytes": os.path.getsize(path), "reads": reads, "runs": runs, "outputs_equal": bool(same)}

result["note"] = ("both arms inflate compressed bytes that lie in host memory into host memory; the device arm includes the rows, upload, "
                  "the copy back and the host's CRC-32; measured once, no rate is promised")
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(result, fh, indent=1)
print(json.dumps({n: {k: t[k] for k in ("ms_per_call", "text_mb_per_second", "kernel_ms_per_call", "kernel_text_mb_per_second",
                                        "device_faster_by_more_than_both_iqr", "host_faster_by_more_than_both_iqr", "stats")}
                  for n, t in result["inputs"].items()}))
if "cli_pair" in result:
    print(json.dumps(result["cli_pair"]))
