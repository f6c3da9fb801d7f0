#!/usr/bin/env python3
"""What follows the contigs of a paired chunk -- formatting, the report lines, collapse -- on the device where the contigs lie,
against the host's functions on the slots that came down.  Every arm begins with the same Engine.contigs_filter_fastq call over
the chunk's two texts (index, pair, build and filter on the device), because the device tail reads the generation that call leaves.

  (a) the call + fastio.format_parallel (fasta, qual) + fastio.format_report on 16 threads;
  (b) the call + resident Engine.format_text (fasta, qual) + Engine.format_report, as plain text;
  (c) (a) + Engine.bgzf_compress of each of the three texts;
  (d) (b) with bgzf=True: only BGZF members come back;
  (e) the call + fastio.Collapse.add of the chunk (the host hashes and looks up every contig);
  (f) the call + resident Engine.collapse_text + Collapse.add(hash=, rep=);
  and the contig call alone (z), and the kernels' own times from the context's events (rounds of their own).

Input: the first pairs of tests/golden (test1.fastq.gz / test2.fastq.bz2, 2 x 251 bases) tiled to `--pairs` pairs (default
65,536, one chunk of the CLI).  One untimed round, then `--rounds` interleaved rounds timed by the wall clock around the
synchronous calls; median, minimum, maximum and interquartile range per arm.  The arms' results are compared once.  Results: one
JSON file (profiles/device_pair_tail_rate.json); nothing here is a threshold, and no rate is promised.
"""
import argparse
import bz2
import gzip
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from moira_amd import fastio as F  # noqa: E402
from moira_amd.engine import Engine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=65536)
ap.add_argument("--rounds", type=int, default=20)
ap.add_argument("--threads", type=int, default=16)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_pair_tail_rate.json"))
args = ap.parse_args()

gold = (gzip.open(os.path.join(ROOT, "tests", "golden", "test1.fastq.gz")).read(), bz2.open(os.path.join(ROOT, "tests", "golden", "test2.fastq.bz2")).read())
per = gold[0].count(b"\n") // 4


def tiled(text):
    whole = text * (args.pairs // per) + b"\n".join(text.split(b"\n")[:4 * (args.pairs % per)]) + (b"\n" if args.pairs % per else b"")
    assert whole.count(b"\n") == 4 * args.pairs
    return whole


ftext, rtext = tiled(gold[0]), tiled(gold[1])
KINDS = (F.FMT_FASTA, F.FMT_QUAL)


def spread(v):
    q = statistics.quantiles(v, n=4)
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "iqr": q[2] - q[0]}


def verdict(sp, host, device):
    both = sp[host]["iqr"] + sp[device]["iqr"]
    return {"device_faster_by_more_than_both_iqr": bool(sp[host]["median"] - sp[device]["median"] > both),
            "host_faster_by_more_than_both_iqr": bool(sp[device]["median"] - sp[host]["median"] > both)}


result = {"pairs": args.pairs, "text_bytes": [len(ftext), len(rtext)], "rounds": args.rounds, "host_threads": args.threads}
pool = ThreadPoolExecutor(args.threads)
with Engine(0) as eng:
    def contigs():
        res = eng.contigs_filter_fastq(ftext, rtext, max_records=args.pairs + 16)
        assert res.n_built == args.pairs and res.n_handed_back == 0 and res.resident > 0
        return res, np.arange(res.n_built, dtype=np.int64)

    def host_texts(res, sel):
        return [b"".join(bytes(p) for p in F.format_parallel(pool, args.threads, res.cbuf, res.cidx, sel, k, scratch="t%d_" % k)) for k in KINDS] \
            + [bytes(F.format_report(res.cbuf, res.cidx, sel, res.aux))]

    def a_host_text():
        res, sel = contigs()
        return [[bytes(p) for p in F.format_parallel(pool, args.threads, res.cbuf, res.cidx, sel, k, scratch="t%d_" % k)] for k in KINDS] \
            + [[bytes(F.format_report(res.cbuf, res.cidx, sel, res.aux))]]

    def b_device_text(bgzf=False):
        res, _ = contigs()
        return [eng.format_text(idx=res.cidx, kind=k, resident=res.resident, bgzf=bgzf) for k in KINDS] \
            + [eng.format_report(idx=res.cidx, resident=res.resident, bgzf=bgzf)]

    def c_host_compressed():
        res, sel = contigs()
        return [eng.bgzf_compress(t) for t in host_texts(res, sel)]

    def collapse(device):
        res, _ = contigs()
        groups = F.Collapse(args.threads)
        try:
            h, rep = eng.collapse_text(resident=res.resident, n=res.n_built) if device else (None, None)
            groups.add(res.cbuf, res.cidx, res.ee, res.has_n, 0, res.aux, hash=h, rep=rep)
            return [np.asarray(x).copy() for x in groups.export()]
        finally:
            groups.close()
    arms = {"z_contig_call_alone": lambda: contigs()[0].n_built,
            "a_host_format_report": a_host_text, "b_device_format_report": b_device_text,
            "c_host_format_report_device_compress": c_host_compressed, "d_device_format_report_compressed": lambda: b_device_text(True),
            "e_host_collapse": lambda: collapse(False), "f_device_collapse": lambda: collapse(True)}

    def run(arm):
        t = time.perf_counter()
        out = arms[arm]()
        return out, (time.perf_counter() - t) * 1e3
    first = {arm: run(arm)[0] for arm in arms}               # untimed: pages are touched, buffers grow
    assert [b"".join(p) for p in first["a_host_format_report"]] == first["b_device_format_report"]
    assert [bytes(x) for x in first["d_device_format_report_compressed"]] == [bytes(x) for x in first["c_host_format_report_device_compress"]]
    assert all(np.array_equal(x, y) for x, y in zip(first["e_host_collapse"], first["f_device_collapse"]))
    result["formatted_bytes"] = [len(t) for t in first["b_device_format_report"]]
    result["groups"] = int(len(first["e_host_collapse"][0]))
    del first
    ms = {arm: [] for arm in arms}
    for _ in range(args.rounds):
        for arm in arms:
            ms[arm].append(run(arm)[1])
    # the kernels' own times, from the context's events
    eng.timing(True)
    kernels = {}
    for arm in ("z_contig_call_alone", "b_device_format_report", "d_device_format_report_compressed", "f_device_collapse"):
        eng.timing_reset()
        for _ in range(3):
            arms[arm]()
        kernels[arm] = {k: round(v[0] / 3.0, 3) for k, v in eng.kernel_times().items() if v[1]}
    # what the ee suffix adds to the three format kernels: the same uploaded fasta call without and with ee
    res, sel = contigs()
    cbuf, cidx, ee = bytes(res.cbuf), res.cidx, np.where(np.isfinite(res.ee), res.ee, 0.0)
    suffix = {}
    for name, kw in (("without_ee", {}), ("with_ee", dict(ee=ee))):
        eng.format_text(cbuf, cidx, kind=F.FMT_FASTA, **kw)
        eng.timing_reset()
        for _ in range(5):
            eng.format_text(cbuf, cidx, kind=F.FMT_FASTA, **kw)
        suffix[name] = round(eng.kernel_times()["pack_text"][0] / 5.0, 3)
    eng.timing(False)
pool.shutdown()
sp = {arm: spread(v) for arm, v in ms.items()}
result.update({
    "ms": ms, "ms_per_call": sp, "kernel_ms_per_call": kernels, "format_kernels_ms_fasta_uploaded": suffix,
    "text_device_against_host": verdict(sp, "a_host_format_report", "b_device_format_report"),
    "compressed_device_against_host": verdict(sp, "c_host_format_report_device_compress", "d_device_format_report_compressed"),
    "collapse_device_against_host": verdict(sp, "e_host_collapse", "f_device_collapse"),
    "note": ("every arm but (z) includes the contigs_filter_fastq call of the chunk, whose slots and arrays come down in every arm; every "
             "arm ends with its output in host memory; measured once, no rate is promised")})
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(result, fh, indent=1)
print(json.dumps({k: result[k] for k in ("pairs", "formatted_bytes", "groups", "ms_per_call", "kernel_ms_per_call", "format_kernels_ms_fasta_uploaded", "text_device_against_host",
                                         "compressed_device_against_host", "collapse_device_against_host")}))
