#!/usr/bin/env python3
"""MPB_FLAG_ODDS against the bit-exact mode and MPB_FLAG_FAST_FMA on BASELINE config 2's resident batch (10 M reads x 300 bases,
sorted pipeline): wall time per step (back-to-back calls, one synchronisation at the end; the modes take turns, `rounds` times,
so that drift shows as spread instead of as a difference), per-kernel times from the library's spans, and the reads each mode
hands to the three-rounding pass (n_overflow).  One JSON line: the figures of ODDS_MODE.md and profiles/odds_rate.json.

    python tools/odds_rate.py [reads] [steps] [rounds] [modes, e.g. exact,fast_fma: what a library from before the flag can run]
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
stride, L = 320, 300
MODES = [("exact", {}), ("fast_fma", dict(fast_fma=True)), ("odds", dict(odds=True))]
if len(sys.argv) > 4:
    MODES = [m for m in MODES if m[0] in sys.argv[4].split(",")]

with Engine(0) as eng:
    d_q = eng.alloc(n * stride)
    d_ee, d_ns, d_pass = eng.alloc(n * 8), eng.alloc(n * 4), eng.alloc(n)
    eng.synth_fill(d_q, n, stride, fixed_len=L, seed=2)
    run = lambda prm, counts=False: eng.filter_device(d_q, n, stride, fixed_len=L, d_ee=d_ee, d_ns=d_ns, d_pass=d_pass,
                                                      params=prm, want_counts=counts)
    prm = {name: eng.params(alpha=0.005, uncert=0.01, ambigs="treat_as_errors", no_narrow=True, **kw) for name, kw in MODES}
    out = {"tool": "odds_rate", "reads": n, "bases": L, "stride": stride, "steps": steps, "rounds": rounds,
           "library": os.environ.get("MOIRA_PB_LIB", "in-tree"), "modes": {}}
    ee_exact = None
    for name, _ in MODES:
        c = run(prm[name], True)                    # warm-up of the mode's kernels, and its counts
        ee = d_ee.download(np.float64, n)
        m = out["modes"][name] = {"n_pass": int(c.n_pass), "n_overflow": int(c.n_overflow), "step_ms": []}
        if ee_exact is None:
            ee_exact = ee
        else:
            fin = np.isfinite(ee_exact) & (ee_exact != 0)
            assert np.array_equal(np.isnan(ee), np.isnan(ee_exact))
            m["worst_rel_vs_exact"] = float((np.abs(ee[fin] - ee_exact[fin]) / np.abs(ee_exact[fin])).max())
            m["reads_with_other_bits"] = int((ee[fin] != ee_exact[fin]).sum())
            m["n_pass_equal"] = bool(c.n_pass == out["modes"]["exact"]["n_pass"])
    for _ in range(rounds):
        for name, _kw in MODES:
            run(prm[name]); eng.synchronize()
            t0 = time.perf_counter()
            for _s in range(steps):
                run(prm[name])
            eng.synchronize()
            out["modes"][name]["step_ms"].append(round((time.perf_counter() - t0) * 1e3 / steps, 4))
    for name, _kw in MODES:
        eng.timing(True); eng.timing_reset()
        for _s in range(5):
            run(prm[name])
        out["modes"][name]["kernel_ms"] = {k: round(v[0] / 5.0, 4) for k, v in sorted(eng.kernel_times().items()) if v[1]}
        eng.timing(False)
        ms = out["modes"][name]["step_ms"]
        out["modes"][name]["step_ms_median"] = float(np.median(ms))
print(json.dumps(out))
