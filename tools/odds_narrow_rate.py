#!/usr/bin/env python3
"""MPB_FLAG_ODDS_NARROW (the one-FMA form of the natural-order narrow pass) against the exact narrow pass and MPB_FLAG_ODDS alone
(sorted pipeline), on the 10 M x 300 clean batch (seed 2, profile 1), the 5 M ragged clean batch of bench_extras'
high_quality_ragged, and mixes of the clean batch with 5 / 20 / 40 % of BASELINE's reads (blocks of 1024 reads spread evenly).
Wall time per step (back-to-back calls, one synchronisation at the end; the options take turns, `rounds` times, so that drift
shows as spread instead of as a difference), kernel times from the library's spans, n_fallback, n_overflow, the worst relative
error against the exact call and whether n_pass is equal.  One JSON line: the figures of ODDS_MODE.md "The narrow passes" and
profiles/odds_narrow_rate.json, and what narrow_rows_from_sample's constants for this mode are fitted to.

    python tools/odds_narrow_rate.py [reads of the fixed batch] [steps] [rounds] [reads of the ragged batch]
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from moira_amd.engine import Engine  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 3
n_rag = int(sys.argv[4]) if len(sys.argv) > 4 else 5_000_000
ON = dict(odds=True, odds_narrow=True)
OPTIONS = [("exact_narrow", {}), ("odds_sorted", dict(odds=True)), ("odds_narrow_choice", ON),
           ("odds_narrow_r2", dict(narrow_rows=2, **ON)), ("odds_narrow_r3", dict(narrow_rows=3, **ON)),
           ("odds_narrow_r4", dict(narrow_rows=4, **ON))]
BLOCK = 1024


def measure(eng, run, options, want_error=True):
    """options: [(name, params)] -> {name: figures}; the first option is the exact reference of the error columns."""
    out, ee_exact, n_pass_exact = {}, None, None
    for name, prm in options:
        c = run(prm, True)                                  # warm-up, counts, and (the choice) the sample
        path = eng.last_path()
        m = out[name] = {"n_pass": int(c.n_pass), "n_overflow": int(c.n_overflow), "narrow_rows": path["narrow_rows"],
                         "n_fallback": int(path["n_fallback"]), "step_ms": []}
        if not want_error:
            continue
        ee = run.download()
        if ee_exact is None:
            ee_exact, n_pass_exact = ee, c.n_pass
        else:
            fin = np.isfinite(ee_exact) & (ee_exact != 0)
            m["nan_equal"] = bool(np.array_equal(np.isnan(ee), np.isnan(ee_exact)))
            m["worst_rel_vs_exact"] = float((np.abs(ee[fin] - ee_exact[fin]) / np.abs(ee_exact[fin])).max())
            m["reads_with_other_bits"] = int((ee[fin] != ee_exact[fin]).sum())
            m["n_pass_equal"] = bool(c.n_pass == n_pass_exact)
    for _ in range(rounds):
        for name, prm in options:
            run(prm); eng.synchronize()
            t0 = time.perf_counter()
            for _s in range(steps):
                run(prm)
            eng.synchronize()
            out[name]["step_ms"].append(round((time.perf_counter() - t0) * 1e3 / steps, 4))
    for name, prm in options:
        eng.timing(True); eng.timing_reset()
        for _s in range(5):
            run(prm)
        out[name]["kernel_ms"] = {k: round(v[0] / 5.0, 4) for k, v in sorted(eng.kernel_times().items()) if v[1]}
        eng.timing(False)
        out[name]["step_ms_median"] = float(np.median(out[name]["step_ms"]))
    return out


with Engine(0) as eng:
    prm = [(name, eng.params(alpha=0.005, uncert=0.01, ambigs="treat_as_errors", **kw)) for name, kw in OPTIONS]
    out = {"tool": "odds_narrow_rate", "steps": steps, "rounds": rounds, "block": BLOCK}

    # ---- the fixed-length batch, clean and mixed
    stride, L = 320, 300
    d_q, d_ee, d_ns, d_pass = eng.alloc(n * stride), eng.alloc(n * 8), eng.alloc(n * 4), eng.alloc(n)

    def run(p, counts=False):
        return eng.filter_device(d_q, n, stride, fixed_len=L, d_ee=d_ee, d_ns=d_ns, d_pass=d_pass, params=p, want_counts=counts)
    run.download = lambda: d_ee.download(np.float64, n)
    eng.synth_fill(d_q, n, stride, fixed_len=L, seed=2, profile=1)
    out["clean"] = {"reads": n, "bases": L, "stride": stride, "options": measure(eng, run, prm)}
    nblk = n // BLOCK
    for pct in (5, 20, 40):
        # blocks k with floor(k pct / 100) != floor((k - 1) pct / 100) hold BASELINE's reads: pct % of the blocks, spread evenly
        eng.synth_fill(d_q, n, stride, fixed_len=L, seed=2, profile=1)
        bad = [k for k in range(1, nblk) if (k * pct) // 100 != ((k - 1) * pct) // 100]
        for k in bad:
            eng.synth_fill(d_q.ptr + k * BLOCK * stride, BLOCK, stride, fixed_len=L, seed=2, first_read=k * BLOCK, profile=0)
        eng.synchronize()
        out["mix_%d" % pct] = {"reads": n, "bad_reads": len(bad) * BLOCK,
                               "options": measure(eng, run, prm, want_error=False)}
    for b in (d_q, d_ee, d_ns, d_pass):
        b.free()

    # ---- the ragged clean batch
    stride = 640
    d_q, d_ee, d_ns, d_pass, d_len = (eng.alloc(n_rag * stride), eng.alloc(n_rag * 8), eng.alloc(n_rag * 4), eng.alloc(n_rag),
                                      eng.alloc(n_rag * 4))
    eng.synth_fill(d_q, n_rag, stride, min_len=50, max_len=600, d_len=d_len, seed=6, profile=1)

    def run_rag(p, counts=False):
        return eng.filter_device(d_q, n_rag, stride, d_len=d_len, d_ee=d_ee, d_ns=d_ns, d_pass=d_pass, params=p, want_counts=counts)
    run_rag.download = lambda: d_ee.download(np.float64, n_rag)
    out["ragged"] = {"reads": n_rag, "min_len": 50, "max_len": 600, "stride": stride, "options": measure(eng, run_rag, prm)}
print(json.dumps(out))
