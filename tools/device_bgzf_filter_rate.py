#!/usr/bin/env python3
"""BGZF FASTQ filtered where it inflates against the two-call ways, for compressed bytes that are already in host memory.

  (a) host inflate + filter_fastq:    libmoira_io's mio_bgzf_inflate_mt on 16 threads, then Engine.filter_fastq (the text goes up once);
  (b) device inflate + filter_fastq:  Engine.bgzf_inflate (the text comes down, CRC on the host), then Engine.filter_fastq (it goes up again);
  (c) fused, with the text:           Engine.filter_bgzf_fastq (compressed bytes up; inflate, CRC, index, pack, filter; text down once);
  (d) fused, text=False:              the same without the text coming back;
  the kernels alone, from the context's own events (rounds of their own): k_bgzf_crc32 from a crc32_ranges call over the same
  members, and inflate + CRC, the index and the pack from a fused call; zlib.crc32 over the same members on the same host threads
  beside them (the library's own bgzf_crc32 is not exported).

Input: the text of tests/golden/test1.fastq.gz (1,000 reads of 251 bases) tiled to `--mib` MiB (default 256), compressed once by
cli.bgzf_compress at level 4.  The text of every arm that brings one lands in ONE buffer that is touched before the first round
(text= / out=): a copy into fresh pages costs several times the copy itself, on either side.  One untimed round, then `--rounds`
interleaved rounds of the arms timed by the wall clock around the synchronous calls; median, minimum, maximum and interquartile
range per arm.  The arms' results are compared once.  Then one pair of CLI runs at -p 16 (BGZF FASTQ in, FASTQ out, -c false; with and without --device_inflate --device_index --device_pack), each in
a process of its own, outputs compared.  Results: one JSON file (profiles/device_bgzf_filter_rate.json); nothing here is a
threshold, and no rate is promised.
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
import zlib
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_bgzf_filter_rate.json"))
args = ap.parse_args()

golden = gzip.open(os.path.join(ROOT, "tests", "golden", "test1.fastq.gz")).read()
size = args.mib << 20
text = (golden * (size // len(golden) + 1))[:size]
text = text[:text.rfind(b"\n@") + 1]                         # whole records: the CLI pairs read the same bytes
reads = text.count(b"\n") // 4
cap = reads + 16
blob = cli.bgzf_compress(text, 4)
sizes = []
at = 0
while at < len(blob):
    sizes.append(int.from_bytes(blob[at + 16:at + 18], "little") + 1)
    at += sizes[-1]
sizes = np.array(sizes, np.int32)
offs = np.cumsum(sizes, dtype=np.int64) - sizes
out_offs = np.minimum(np.arange(len(sizes) + 1, dtype=np.int64) * cli.BGZF_DATA, len(text))
data = np.frombuffer(blob + bytes(8), np.uint8)[:len(blob)]  # (eight readable bytes behind the end: the host decoder reads whole words)
io_lib = F.load()


text_buf = np.zeros(len(text), np.uint8)                     # every arm's text lands in this one buffer, touched before the first round


def host_inflate():
    out = text_buf
    rc = io_lib.mio_bgzf_inflate_mt(data.ctypes.data, offs.ctypes.data, sizes.ctypes.data, out_offs.ctypes.data, len(sizes),
                                    out.ctypes.data, args.threads)
    assert rc >= 0
    return out


def spread(v):
    q = statistics.quantiles(v, n=4)
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "iqr": q[2] - q[0]}


def verdict(sp, a, b):
    both = sp[a]["iqr"] + sp[b]["iqr"]
    return {"%s_faster_by_more_than_both_iqr" % b: bool(sp[a]["median"] - sp[b]["median"] > both),
            "%s_faster_by_more_than_both_iqr" % a: bool(sp[b]["median"] - sp[a]["median"] > both)}


def same(x, y):
    return (np.array_equal(x.idx, y.idx) and x.consumed == y.consumed and np.array_equal(x.ee.view(np.uint64), y.ee.view(np.uint64))
            and np.array_equal(x.ns, y.ns) and np.array_equal(x.passed, y.passed) and np.array_equal(x.lens, y.lens)
            and np.array_equal(x.has_n, y.has_n))


result = {"text_bytes": len(text), "compressed_bytes": len(blob), "members": len(sizes), "reads": reads, "rounds": args.rounds,
          "host_threads": args.threads}
with Engine(0) as eng:
    arms = {
        "host_inflate_filter_fastq": lambda: eng.filter_fastq(host_inflate(), True, cap),
        "device_inflate_filter_fastq": lambda: eng.filter_fastq(eng.bgzf_inflate(data, offs, sizes, out_offs, out=text_buf)[0], True, cap),
        "fused_with_text": lambda: eng.filter_bgzf_fastq(data, offs, sizes, out_offs, max_records=cap, text=text_buf),
        "fused_without_text": lambda: eng.filter_bgzf_fastq(data, offs, sizes, out_offs, max_records=cap, text=False),
    }
    first = {k: fn() for k, fn in arms.items()}              # untimed: pages are touched, buffers grow
    ref = first["host_inflate_filter_fastq"]
    assert len(ref.idx) == reads and ref.bad is None and ref.consumed == len(text)
    assert all(same(ref, r) for r in first.values()) and text_buf.tobytes() == text
    assert first["fused_without_text"].text is None and first["fused_with_text"].member_stats["taken"] == len(sizes)
    del first, ref
    ms = {k: [] for k in arms}
    for _ in range(args.rounds):
        for arm, fn in arms.items():
            t = time.perf_counter()
            fn()
            ms[arm].append((time.perf_counter() - t) * 1e3)
    # the kernels alone: the context's events
    lens = np.diff(out_offs).astype(np.int32)
    want_crc = np.array([zlib.crc32(text[a:b]) for a, b in zip(out_offs[:-1].tolist(), out_offs[1:].tolist())], np.uint32)
    eng.timing(True)
    eng.timing_reset()
    for _ in range(3):
        assert np.array_equal(eng.crc32_ranges(text, out_offs[:-1], lens), want_crc)
    crc_kernel_ms = eng.kernel_times()["bgzf_inflate"][0] / 3.0
    eng.timing_reset()
    for _ in range(3):
        eng.filter_bgzf_fastq(data, offs, sizes, out_offs, max_records=cap, text=False)
    fused_kernel_ms = {k: round(v[0] / 3.0, 3) for k, v in sorted(eng.kernel_times().items()) if v[1]}
    eng.timing(False)
    mv = memoryview(text)
    pairs = list(zip(out_offs[:-1].tolist(), out_offs[1:].tolist()))
    part = [pairs[k::args.threads] for k in range(args.threads)]
    host_crc_ms = []
    with ThreadPoolExecutor(args.threads) as pool:
        for _ in range(5):
            t = time.perf_counter()
            list(pool.map(lambda ps: [zlib.crc32(mv[a:b]) for a, b in ps], part))
            host_crc_ms.append((time.perf_counter() - t) * 1e3)
    sp = {k: spread(v) for k, v in ms.items()}
    result.update({
        "ms": ms, "ms_per_call": sp,
        "text_mb_per_second": {k: len(text) / 1e6 / (v["median"] * 1e-3) for k, v in sp.items()},
        "fused_with_text_against_host_inflate": verdict(sp, "host_inflate_filter_fastq", "fused_with_text"),
        "fused_without_text_against_host_inflate": verdict(sp, "host_inflate_filter_fastq", "fused_without_text"),
        "fused_with_text_against_device_inflate": verdict(sp, "device_inflate_filter_fastq", "fused_with_text"),
        "crc_kernel_ms_per_call": round(crc_kernel_ms, 3),
        "crc_kernel_text_mb_per_second": len(text) / 1e6 / (crc_kernel_ms * 1e-3) if crc_kernel_ms else None,
        "host_zlib_crc32_ms_on_threads": spread(host_crc_ms),
        "fused_kernel_ms_per_call": fused_kernel_ms})

if not args.no_cli:
    # one pair of CLI runs, a process each: seconds of the whole run
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "tiled.fastq.gz")
        with open(path, "wb") as fh:
            fh.write(blob + cli.BGZF_EOF)
        runs = {}
        p = args.threads
        for label, extra in (("host", []), ("device", ["--device_inflate", "--device_index", "--device_pack"])):
            cmd = [sys.executable, os.path.join(ROOT, "moira.py"), "-ffq", path, "-op", os.path.join(td, label), "--silent", "-c", "false",
                   "-o", "fastq", "-p", str(p)] + extra
            t = time.perf_counter()
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
            sec = time.perf_counter() - t
            files = sorted(f for f in os.listdir(td) if f.startswith(label + "."))
            runs[label] = {"returncode": r.returncode, "seconds": sec, "reads_per_second": reads / sec,
                           "output_bytes": sum(os.path.getsize(os.path.join(td, f)) for f in files),
                           "files": [f.split(".", 1)[1] for f in files],
                           "messages": [l for l in r.stdout.splitlines() if "--device_" in l]}
        equal = runs["host"]["files"] == runs["device"]["files"] and all(
            open(os.path.join(td, "host." + f), "rb").read() == open(os.path.join(td, "device." + f), "rb").read()
            for f in runs["host"]["files"])
        result["cli_pair"] = {"command": "moira.py -ffq tiled.fastq.gz -c false -o fastq -p %d [--device_inflate --device_index --device_pack]" % p,
                              "input_bytes": len(blob), "reads": reads, "runs": runs, "outputs_equal": bool(equal)}

result["note"] = ("every arm starts from compressed bytes that lie in host memory and ends with the index and the results (and, but for "
                  "the last arm, the text) in host memory; measured once, no rate is promised")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(result, fh, indent=1)
print(json.dumps({k: result[k] for k in result if k not in ("ms", "cli_pair", "note")}))
if "cli_pair" in result:
    print(json.dumps(result["cli_pair"]))
