#!/usr/bin/env python3
"""Packing FASTQ text on the device against packing it on the host, for a chunk that is already in host memory with its index.

  (a) what the CLI does without --device_pack: fastio.pack_parallel + Engine.filter per 64-byte length bucket;
  (b) one Engine.filter_text (mpb_filter_text_host: one upload of the text, k_pack_text, the filter on the ragged matrix).

`--reads` records of `--length` bases (BASELINE's quality model), one process, `--threads` packing threads, `--rounds`
alternating rounds after one untimed round.  Reported: ms per chunk of each round and their medians, the pack_text kernel time
alone and its bytes / time (text read once: 2 x length per record; matrix written once: the row stride) next to k_prepass'
measured 5.0-5.5 TB/s of streaming, equality of the two results.  Then the CLI end to end on files made of the same reads:
"fastq in, fastq out, no collapse, -p threads" and the paired run (contigs + filter, no collapse) of tools/cli_throughput.py,
each with and without --device_pack.  Results: one JSON file (profiles/device_pack_rate.json); nothing here is a threshold.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import numpy as np  # noqa: E402
import pb_oracle as O  # noqa: E402
from moira_amd import cli  # noqa: E402
from moira_amd import fastio as F  # noqa: E402
from moira_amd.buckets import bucket_of  # noqa: E402
from moira_amd.engine import Engine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=2_000_000)
ap.add_argument("--length", type=int, default=250)
ap.add_argument("--threads", type=int, default=16)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--pairs", type=int, default=200_000)
ap.add_argument("--skip-cli", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_pack_rate.json"))
args = ap.parse_args()
n, Lr, T = args.reads, args.length, args.threads


def fastq_bytes(prefix, bases, quals):
    """m records of equal length as one byte matrix (fixed-width decimal ids) -> uint8 array of the file's text."""
    m, L = bases.shape
    w = len(str(m - 1))
    ids = np.char.zfill(np.arange(m).astype("U%d" % w), w).astype("S%d" % w).view(np.uint8).reshape(m, w)
    head = np.frombuffer(("@" + prefix).encode(), np.uint8)
    rec = np.empty((m, len(head) + w + 1 + L + 3 + L + 1), np.uint8)
    c = 0
    for part in (head, ids, b"\n", bases, b"\n+\n", quals, b"\n"):
        part = np.frombuffer(part, np.uint8) if isinstance(part, bytes) else part
        k = part.shape[-1]
        rec[:, c:c + k] = part
        c += k
    return rec.reshape(-1)


q, _ = O.synth_fill(n, (Lr + 15) // 16 * 16, fixed_len=Lr, seed=1)
rng = np.random.default_rng(1)
bases = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (n, Lr))]
bases[q[:, :Lr] == 0] = ord("N")
quals = (np.maximum(q[:, :Lr], 1) + 33).astype(np.uint8)
text = fastq_bytes("r", bases, quals)
idx, consumed, err = F.index(text, True, n, threads=T)
assert err is None and len(idx) == n and consumed == len(text)
result = {"reads": n, "read_length": Lr, "threads": T, "rounds": args.rounds, "text_bytes": int(len(text)), "host_pack": [], "filter_text": []}

from concurrent.futures import ThreadPoolExecutor  # noqa: E402
pool = ThreadPoolExecutor(T) if T > 1 else None
with Engine(0) as eng:
    lens = idx[:, F.SEQ_LEN].copy()

    def host_pack():
        """(a) -> (ee, has_n)"""
        strides = bucket_of(lens, 64)
        ee, has_n = np.zeros(n, np.float64), np.zeros(n, bool)
        for stride in np.unique(strides):
            sel = np.nonzero(strides == stride)[0]
            qm, ln, fl = F.pack_parallel(pool, T, text, idx, sel, 33, 0, False, int(stride))
            ee[sel] = eng.filter(qm, lens=ln, uncert=1.0).ee
            has_n[sel] = fl
        return ee, has_n

    def device_pack():
        """(b) -> (ee, has_n)"""
        r = eng.filter_text(text, idx, uncert=1.0)
        return r.ee, r.has_n

    a, b = host_pack(), device_pack()                               # untimed: buffers grow, pages are touched
    result["results_equal"] = bool(np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64)) and np.array_equal(a[1], b[1]))
    for _ in range(args.rounds):
        for name, fn in (("host_pack", host_pack), ("filter_text", device_pack)):
            t = time.perf_counter()
            fn()
            result[name].append((time.perf_counter() - t) * 1e3)
    eng.timing(True)
    eng.timing_reset()
    for _ in range(args.rounds):
        device_pack()
    ms, launches = eng.kernel_times()["pack_text"]
    eng.timing(False)
    stride = (Lr + 127) // 128 * 128
    moved = n * (2 * Lr + stride + 24 + 5)                          # text read once, matrix written once, descriptors, len + flag
    result["median_ms_per_chunk"] = {k: statistics.median(result[k]) for k in ("host_pack", "filter_text")}
    result["pack_text_kernel"] = {"ms_per_launch": ms / max(launches, 1), "launches": int(launches), "bytes_moved": int(moved),
                                  "TB_per_s": moved / (ms / max(launches, 1) * 1e-3) / 1e12 if ms > 0 else None,
                                  "yardstick": "k_prepass streams at 5.0-5.5 TB/s"}
if pool is not None:
    pool.shutdown()

if not args.skip_cli:
    tmp = tempfile.mkdtemp(dir=os.environ.get("CLI_TMP") or None)
    path = os.path.join(tmp, "synth.fastq")
    text.tofile(path)

    def paired_files(m, L=Lr, frag=380):
        """m pairs of 2 x L bp reads off random fragments, ~1 % substitutions (tools/cli_throughput.py's)."""
        g = np.random.default_rng(7)
        B = np.frombuffer(b"ACGT", np.uint8)
        lut = np.zeros(256, np.uint8)
        for x, y in zip(b"ACGT", b"TGCA"):
            lut[x] = y
        frags = B[g.integers(0, 4, (m, frag))]
        fwd, rev = frags[:, :L].copy(), lut[frags[:, frag - L:][:, ::-1]]
        for arr in (fwd, rev):
            pos = np.minimum((g.random((m, 3)) ** 0.4 * L).astype(int), L - 1)
            arr[np.arange(m)[:, None], pos] = B[g.integers(0, 4, (m, 3))]
        paths = []
        for tag, arr in (("R1", fwd), ("R2", rev)):
            pth = os.path.join(tmp, "synth_%s.fastq" % tag)
            fastq_bytes("p", arr, quals[:m]).tofile(pth)
            paths.append(pth)
        return paths

    def run(label, count, argv):
        out = os.path.join(tmp, "out")
        a = cli.parse_arguments(argv + ["-op", out, "--silent"])
        t = time.perf_counter()
        rc = cli.main(a, out=open(os.devnull, "w"))
        dt = time.perf_counter() - t
        for f in os.listdir(tmp):                                   # (the next run is not measured under write-back throttling)
            if f.startswith("out."):
                os.remove(os.path.join(tmp, f))
        os.sync()
        print("CLI end to end [%s]: %d records in %.2f s = %.0f /s; rc=%d" % (label, count, dt, count / dt, rc), flush=True)
        return {"seconds": dt, "per_second": count / dt, "rc": rc}

    m = min(n, args.pairs)
    r1, r2 = paired_files(m)
    single = ["-ffq", path, "-c", "false", "-o", "fastq", "-p", str(T)]
    paired = ["-ffq", r1, "-rfq", r2, "--paired", "-c", "false", "-p", str(T)]
    run("warm-up", n, single)
    result["cli"] = {}
    for rnd in range(args.rounds):
        for name, count, argv in (("fastq in, fastq out, no collapse, -p %d" % T, n, single),
                                  ("paired 2x%d: contigs + filter, no collapse" % Lr, m, paired)):
            for sw in (False, True):
                key = name + (" --device_pack" if sw else "")
                result["cli"].setdefault(key, []).append(run(key, count, argv + (["--device_pack"] if sw else [])))
    import shutil
    shutil.rmtree(tmp, ignore_errors=True)

with open(args.out, "w") as f:
    json.dump(result, f, indent=1)
print(json.dumps({k: result[k] for k in ("median_ms_per_chunk", "pack_text_kernel", "results_equal")}))
