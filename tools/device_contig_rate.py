#!/usr/bin/env python3
"""Building paired-read contigs on the device against building them on the host, for a chunk that is already in host memory with
its two record indexes.

  (a) moira_amd.contig.contigs_from_fastq on `--threads` host threads (libmoira_contig.so: what the CLI does by default);
  (b) Engine.contigs_text (mpb_contigs_text_host: both texts uploaded once, k_contig per size class, the slots copied back).

Input: the golden paired inputs (tests/golden/test1.fastq.gz + test2.fastq.bz2, 1,000 pairs), tiled to a chunk of
cli.PAIR_CHUNK_READS pairs.  Both calls are synchronous; `--rounds` alternating rounds after one untimed round.  Reported: ms
per chunk of each round, their medians and the pairs per second they amount to, the share of pairs the device handed back, and
equality of the two results on the pairs the device built.  Results: one JSON file (profiles/device_contig_rate.json); nothing
here is a threshold, and no rate is promised.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from moira_amd import cli  # noqa: E402
from moira_amd import contig as CT  # noqa: E402
from moira_amd import fastio as F  # noqa: E402
from moira_amd.engine import Engine  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=cli.PAIR_CHUNK_READS)
ap.add_argument("--threads", type=int, default=16)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_contig_rate.json"))
args = ap.parse_args()

ffh, rfh = cli.open_input_binary(os.path.join(GOLD, "test1.fastq.gz"), 1), cli.open_input_binary(os.path.join(GOLD, "test2.fastq.bz2"), 1)
try:
    (fbuf, fidx, rbuf, ridx), = list(F.PairedFastqChunks(ffh, rfh, 65536, threads=1))
finally:
    ffh.close()
    rfh.close()
fbuf, rbuf = np.frombuffer(bytes(fbuf), np.uint8), np.frombuffer(bytes(rbuf), np.uint8)
m, n = len(fidx), args.pairs
reps = (n + m - 1) // m


def tiled(buf, idx):
    """The chunk's text `reps` times over, the index rows shifted along -> (text, index of the first n records)."""
    out = np.tile(np.asarray(idx, np.int64), (reps, 1))
    out[:, [F.HDR_OFF, F.SEQ_OFF, F.QUAL_OFF]] += (np.repeat(np.arange(reps, dtype=np.int64), len(idx)) * len(buf))[:, None]
    return np.tile(buf, reps), np.ascontiguousarray(out[:n])


ftext, fi = tiled(fbuf, fidx)
rtext, ri = tiled(rbuf, ridx)
result = {"pairs": n, "golden_pairs": m, "threads": args.threads, "rounds": args.rounds,
          "forward_length": {"min": int(fi[:, F.SEQ_LEN].min()), "max": int(fi[:, F.SEQ_LEN].max())},
          "reverse_length": {"min": int(ri[:, F.SEQ_LEN].min()), "max": int(ri[:, F.SEQ_LEN].max())},
          "text_bytes": int(len(ftext) + len(rtext)), "host": [], "device": []}

with Engine(0) as eng:
    host = lambda: CT.contigs_from_fastq(ftext, fi, rtext, ri, 33, threads=args.threads)
    device = lambda: eng.contigs_text(ftext, fi, rtext, ri, 33)
    a, b = host(), device()                                         # untimed: buffers grow, pages are touched
    built = np.nonzero(b.done)[0]
    rows = lambda buf, idx: [bytes(buf[r[0]:r[4] + r[5]]) for r in idx]
    result["handed_back"] = int(b.n_handed_back)
    result["handed_back_share"] = b.n_handed_back / n
    result["results_equal_on_built_pairs"] = bool(np.array_equal(a[1][built], b.cidx[built]) and np.array_equal(a[2][built], b.aux[built]) and
                                                  rows(a[0], a[1][built]) == rows(b.cbuf, b.cidx[built]))
    for _ in range(args.rounds):
        for name, fn in (("host", host), ("device", device)):
            t = time.perf_counter()
            fn()
            result[name].append((time.perf_counter() - t) * 1e3)
result["median_ms_per_chunk"] = {k: statistics.median(result[k]) for k in ("host", "device")}
result["pairs_per_second"] = {k: n / (v * 1e-3) for k, v in result["median_ms_per_chunk"].items()}
result["note"] = "device: Engine.contigs_text alone, synchronous, upload and copy-back included; handed-back pairs are NOT rebuilt in its time"
with open(args.out, "w") as f:
    json.dump(result, f, indent=1)
print(json.dumps({k: result[k] for k in ("median_ms_per_chunk", "pairs_per_second", "handed_back_share", "results_equal_on_built_pairs")}))
