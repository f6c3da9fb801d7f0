#!/usr/bin/env python3
"""Hashing and grouping a chunk's reads on the device against the host collapse doing both, for one chunk of the CLI.

  (a) fastio.Collapse.add on 16 threads: hash, look up and compare every read (mio_collapse_add);
  (b) Engine.collapse_text, resident form, behind an Engine.filter_fastq call made outside the timed span, then
      fastio.Collapse.add(hash=, rep=) on 16 threads (mio_collapse_add_grouped); the two parts are also given apart;
  and the three kernels alone, from the context's own events (rounds of their own).

Two texts of `--mib` MiB (default 64: one block of --device_index, so one call of the CLI): the reads of tests/golden/test1.fastq.gz
(1,000 reads of 251 bases) tiled, so that almost every read is a duplicate within the chunk; and the same with one seeded
substitution in every read of every tile but the first, so that most sequences are distinct.  Every timed call fills a fresh
Collapse object (made and destroyed outside the timed span).  One untimed round, then `--rounds` interleaved rounds of the arms
timed by the wall clock around the synchronous calls; median, minimum, maximum and interquartile range per arm.  The arms'
objects are compared once (export arrays).  Then one pair of CLI runs at -p 16 on the tiled text of `--cli_mib` MiB (FASTQ in,
-c true, --device_pack --device_index with and without --device_collapse), each in a process of its own.  Results: one JSON file
(profiles/device_collapse_rate.json); nothing here is a threshold, and no rate is promised.
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
ap.add_argument("--mib", type=int, default=64)
ap.add_argument("--cli_mib", type=int, default=256)
ap.add_argument("--rounds", type=int, default=20)
ap.add_argument("--threads", type=int, default=16)
ap.add_argument("--no_cli", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_collapse_rate.json"))
args = ap.parse_args()

golden = gzip.open(os.path.join(ROOT, "tests", "golden", "test1.fastq.gz")).read()


def tiled(mib):
    size = mib << 20
    text = (golden * (size // len(golden) + 1))[:size]
    return text[:text.rfind(b"\n@") + 1]                     # whole records


def indexed(text):
    reads = text.count(b"\n") // 4
    idx = F.index(text, True, reads + 16, threads=args.threads)[0].copy()
    assert len(idx) == reads
    return idx


def substituted(text, idx):
    """One seeded substitution in every read behind the first tile: most sequences of the chunk become distinct."""
    rng = np.random.default_rng(20)
    a = np.frombuffer(text, np.uint8).copy()
    rows = idx[1000:]
    at = rows[:, F.SEQ_OFF] + rng.integers(0, 1 << 30, len(rows)) % rows[:, F.SEQ_LEN]
    turn = np.zeros(256, np.uint8)
    for i, b in enumerate(b"ACGT"):
        turn[b] = i
    a[at] = np.frombuffer(b"ACGT", np.uint8)[(turn[a[at]] + rng.integers(1, 4, len(rows))) % 4]
    return a.tobytes()


def spread(v):
    q = statistics.quantiles(v, n=4)
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "iqr": q[2] - q[0]}


def verdict(sp, host, device):
    both = sp[host]["iqr"] + sp[device]["iqr"]
    faster, slower = sp[host]["median"] - sp[device]["median"] > both, sp[device]["median"] - sp[host]["median"] > both
    return {"device_faster_by_more_than_both_iqr": bool(faster), "host_faster_by_more_than_both_iqr": bool(slower),
            "says": "faster" if faster else "slower" if slower else "no difference"}


base = tiled(args.mib)
base_idx = indexed(base)
texts = {"duplicates": base, "distinct": substituted(base, base_idx)}
result = {"text_bytes": len(base), "reads": len(base_idx), "rounds": args.rounds, "host_threads": args.threads, "texts": {}}
with Engine(0) as eng:
    for name, text in texts.items():
        idx = indexed(text)
        n = len(idx)
        ee = np.random.default_rng(21).random(n)
        flags = np.zeros(n, np.uint8)
        made = {}

        def host():
            g = F.Collapse(args.threads)
            t = time.perf_counter()
            g.add(text, idx, ee, flags)
            return g, {"a_host_collapse": (time.perf_counter() - t) * 1e3}

        def device():
            g = F.Collapse(args.threads)
            gen = eng.filter_fastq(text, True, n + 16).resident      # outside the timed span: the CLI has made this call anyway
            t0 = time.perf_counter()
            h, rep = eng.collapse_text(resident=gen, n=n)
            t1 = time.perf_counter()
            g.add(text, idx, ee, flags, hash=h, rep=rep)
            t2 = time.perf_counter()
            made["rep"] = rep
            return g, {"b_device_then_grouped": (t2 - t0) * 1e3, "b1_device_call": (t1 - t0) * 1e3, "b2_grouped_add": (t2 - t1) * 1e3}
        ga, gb = host()[0], device()[0]                      # untimed: pages are touched, buffers grow
        assert len(ga) == len(gb) and all(np.array_equal(x, y) for x, y in zip(ga.export(), gb.export()))
        groups, dup_share = len(ga), float(np.mean(made["rep"] != np.arange(n)))
        ga.close(), gb.close()
        ms = {}
        for _ in range(args.rounds):
            for arm in (host, device):
                g, took = arm()
                g.close()
                for k, v in took.items():
                    ms.setdefault(k, []).append(v)
        eng.timing(True)
        eng.timing_reset()
        gen = eng.filter_fastq(text, True, n + 16).resident
        before = eng.kernel_times()["pack_text"][0]
        for _ in range(3):
            eng.collapse_text(resident=gen, n=n)
        kernel_ms = round((eng.kernel_times()["pack_text"][0] - before) / 3.0, 3)
        eng.timing(False)
        sp = {arm: spread(v) for arm, v in ms.items()}
        result["texts"][name] = {
            "reads": n, "groups": groups, "share_of_reads_with_an_earlier_equal_read": dup_share, "ms": ms, "ms_per_call": sp,
            "reads_per_second": {arm: n / (v["median"] * 1e-3) for arm, v in sp.items()},
            "device_then_grouped_against_host": verdict(sp, "a_host_collapse", "b_device_then_grouped"),
            "collapse_kernels_ms_per_call": kernel_ms}

if not args.no_cli:
    with tempfile.TemporaryDirectory() as td:
        text = tiled(args.cli_mib)
        reads = text.count(b"\n") // 4
        path = os.path.join(td, "tiled.fastq")
        with open(path, "wb") as fh:
            fh.write(text)
        runs = {}
        for label, extra in (("host", []), ("device", ["--device_collapse"])):
            cmd = [sys.executable, os.path.join(ROOT, "moira.py"), "-ffq", path, "-op", os.path.join(td, label), "--silent",
                   "-p", str(args.threads), "--device_pack", "--device_index"] + extra
            t = time.perf_counter()
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
            sec = time.perf_counter() - t
            files = sorted(f for f in os.listdir(td) if f.startswith(label + "."))
            runs[label] = {"returncode": r.returncode, "seconds": sec, "reads_per_second": reads / sec,
                           "output_bytes": sum(os.path.getsize(os.path.join(td, f)) for f in files),
                           "files": [f.split(".", 1)[1] for f in files],
                           "messages": [l for l in r.stdout.splitlines() if "--device_" in l]}
        same = runs["host"]["files"] == runs["device"]["files"] and all(
            open(os.path.join(td, "host." + f), "rb").read() == open(os.path.join(td, "device." + f), "rb").read() for f in runs["host"]["files"])
        result["cli_pair"] = {
            "command": "moira.py -ffq tiled.fastq -p %d --device_pack --device_index [--device_collapse]" % args.threads,
            "input_bytes": len(text), "reads": reads, "runs": runs, "outputs_equal": bool(same)}

result["note"] = ("arm (a) starts from text in host memory; arm (b) from what a filter_fastq call outside the timed span left on the device "
                  "(the CLI has made that call anyway) and ends, as (a), with the chunk in a Collapse object; in a CLI run the host collapse "
                  "runs on the writer thread beside the next chunk's filter; measured once, no rate is promised")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(result, fh, indent=1)
print(json.dumps({k: {a: v[a] for a in ("reads", "groups", "ms_per_call", "collapse_kernels_ms_per_call", "device_then_grouped_against_host")}
                  for k, v in result["texts"].items()}))
if "cli_pair" in result:
    print(json.dumps(result["cli_pair"]))
