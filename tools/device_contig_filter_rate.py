#!/usr/bin/env python3
"""Filtering device-built contigs where they lie against bringing them down and sending them up again, for a chunk of pairs that
is already in host memory with its two record indexes.

  (a) two_calls: Engine.contigs_text, then Engine.filter_text on the slot buffer and index that came down (what --device_contigs
      --device_pack did before the fused call existed);
  (b) fused:     Engine.contigs_filter_text (mpb_contigs_filter_text_host: k_contig, k_contig_rows, k_pack_text and the filter
      on the slots in HBM, every copy back at the end).

Input: the golden paired inputs (tests/golden/test1.fastq.gz + test2.fastq.bz2, 1,000 pairs of 2 x 251), tiled to a chunk of
cli.PAIR_CHUNK_READS pairs.  Both arms are synchronous calls timed by the wall clock, interleaved, `--rounds` rounds after one
untimed round.  Reported: ms per chunk of every round, median, minimum, maximum and interquartile range per arm, the pairs
handed back, equality of the two arms' results, arm (a)'s time by its two calls, and -- from rounds of their own with the
context's own timing on -- the time of k_contig, k_contig_rows, k_pack_text and the filter's kernels per chunk.  Results: one JSON file (profiles/device_contig_filter_rate.json); nothing
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
from moira_amd import fastio as F  # noqa: E402
from moira_amd.engine import Engine  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=cli.PAIR_CHUNK_READS)
ap.add_argument("--rounds", type=int, default=20)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_contig_filter_rate.json"))
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
result = {"pairs": n, "golden_pairs": m, "rounds": args.rounds,
          "forward_length": {"min": int(fi[:, F.SEQ_LEN].min()), "max": int(fi[:, F.SEQ_LEN].max())},
          "reverse_length": {"min": int(ri[:, F.SEQ_LEN].min()), "max": int(ri[:, F.SEQ_LEN].max())},
          "text_bytes": int(len(ftext) + len(rtext)), "two_calls": [], "fused": []}

with Engine(0) as eng:
    out = tuple(np.empty(n, dt) for dt in (np.float64, np.int32, np.uint8, np.int32, np.uint8))     # reused, as a streaming caller would

    parts = {"contigs_text": [], "filter_text": []}                  # arm (a) by its two calls

    def two_calls():
        t0 = time.perf_counter()
        r = eng.contigs_text(ftext, fi, rtext, ri, 33)
        t1 = time.perf_counter()
        sel = None if r.n_handed_back == 0 else np.nonzero(r.done)[0]
        f = eng.filter_text(r.cbuf, r.cidx, sel=sel, out=out)
        parts["contigs_text"].append((t1 - t0) * 1e3)
        parts["filter_text"].append((time.perf_counter() - t1) * 1e3)
        return r, f

    def fused():
        return eng.contigs_filter_text(ftext, fi, rtext, ri, 33, out=out)

    (r, f), g = two_calls(), None                                      # untimed: buffers grow, pages are touched
    ref = [np.array(getattr(f, k)) for k in ("ee", "ns", "passed", "lens", "has_n")]
    g = fused()
    built = np.nonzero(r.done)[0]
    result["rec_cap"] = int(r.rec_cap)
    result["slot_bytes"] = int(n * r.rec_cap)
    result["handed_back"] = int(g.n_handed_back)
    result["handed_back_share"] = g.n_handed_back / n
    same = [np.array_equal(np.asarray(getattr(g, k))[built].view(np.uint8), a.view(np.uint8)) for k, a in zip(("ee", "ns", "passed", "lens", "has_n"), ref)]
    result["results_equal"] = bool(all(same) and np.array_equal(g.done, r.done) and np.array_equal(g.filtered, g.done) and
                                   np.array_equal(g.cidx[built], r.cidx[built]) and np.array_equal(g.aux[built], r.aux[built]) and
                                   g.n_pass == f.n_pass and g.filter_error is None)
    assert result["results_equal"], same
    for v in parts.values():
        del v[:]
    for _ in range(args.rounds):
        for name, fn in (("two_calls", two_calls), ("fused", fused)):
            t = time.perf_counter()
            fn()
            result[name].append((time.perf_counter() - t) * 1e3)
    result["two_calls_parts_median_ms"] = {k: statistics.median(v) for k, v in parts.items()}
    # the kernels alone, from the context's own events (a round of its own: the events cost the timed rounds nothing)
    eng.timing(True)
    kernel_ms = {}
    for name, fn in (("two_calls", two_calls), ("fused", fused)):
        eng.timing_reset()
        for _ in range(3):
            fn()
        kernel_ms[name] = {k: round(v[0] / 3.0, 4) for k, v in sorted(eng.kernel_times().items()) if v[1]}
    eng.timing(False)
    result["kernel_ms_per_chunk"] = kernel_ms


def spread(v):
    q = statistics.quantiles(v, n=4)
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "iqr": q[2] - q[0]}


result["ms_per_chunk"] = {k: spread(result[k]) for k in ("two_calls", "fused")}
result["pairs_per_second"] = {k: n / (v["median"] * 1e-3) for k, v in result["ms_per_chunk"].items()}
result["note"] = ("both arms: synchronous calls on one engine, upload and copy-back included, result arrays reused; handed-back pairs "
                  "are NOT rebuilt in either arm's time")
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(result, fh, indent=1)
print(json.dumps({k: result[k] for k in ("ms_per_chunk", "two_calls_parts_median_ms", "pairs_per_second", "handed_back", "results_equal", "kernel_ms_per_chunk")}))
