#!/usr/bin/env python3
"""--error_calc poisson on a RESIDENT batch, start to results in HBM: (i) the composition a caller had before the device tail --
mpb_poisson_lambda_device, D2H of lambda / ns, mpb_poisson_finish_host, H2D of ee / pass -- against (ii) mpb_filter_poisson_device
(k_lambda + k_poisson_tail).  One process; the options take turns over `--rounds` rounds of `--steps` steps (warm-up excluded);
every option ends in a synchronise.  Then the host-fed entry (mpb_filter_poisson_host) with and without
MPB_FLAG_POISSON_DEVICE_TAIL.  Results: one JSON file (profiles/poisson_device_rate.json)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from moira_amd.engine import Engine  # noqa: E402
from moira_amd import _lib as L  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=10_000_000)
ap.add_argument("--host-reads", type=int, default=2_000_000)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "poisson_device_rate.json"))
args = ap.parse_args()
n, stride, Lr = args.reads, 320, 300
result = {"reads": n, "read_length": Lr, "row_stride": stride, "rounds": args.rounds, "steps": args.steps, "warmup": args.warmup,
          "profiles": {}}

with Engine(0) as eng:
    lib, ctx = eng.lib, eng.ctx
    d_q, d_lam, d_ns, d_ee, d_pass = eng.alloc(n * stride), eng.alloc(n * 8), eng.alloc(n * 4), eng.alloc(n * 8), eng.alloc(n)
    d_ee2, d_pass2 = eng.alloc(n * 8), eng.alloc(n)
    h_lam, h_ee = eng.host_alloc(n, np.float64), eng.host_alloc(n, np.float64)          # pinned: the copies run at the link's rate
    h_ns, h_pass = eng.host_alloc(n, np.int32), eng.host_alloc(n, np.uint8)
    prm = eng.params()                                                                    # alpha 0.005, uncert 0.01, treat_as_errors

    def composed():
        """(i) today's composition, results back in HBM; -> n_pass"""
        L.check(lib.mpb_poisson_lambda_device(ctx, d_q.ptr, n, stride, None, Lr, d_lam.ptr, d_ns.ptr))
        L.check(lib.mpb_memcpy_d2h(ctx, h_lam.ctypes.data, d_lam.ptr, n * 8))
        L.check(lib.mpb_memcpy_d2h(ctx, h_ns.ctypes.data, d_ns.ptr, n * 4))
        L.check(lib.mpb_poisson_finish_host(h_lam.ctypes.data, h_ns.ctypes.data, None, Lr, n, C.byref(prm), h_ee.ctypes.data,
                                            h_pass.ctypes.data))
        L.check(lib.mpb_memcpy_h2d(ctx, d_ee.ptr, h_ee.ctypes.data, n * 8))
        L.check(lib.mpb_memcpy_h2d(ctx, d_pass.ptr, h_pass.ctypes.data, n))              # (synchronises)
        return None

    counts = L.FilterCounts()

    def resident():
        """(ii) the resident filter; synchronises inside"""
        L.check(lib.mpb_filter_poisson_device(ctx, d_q.ptr, n, stride, None, Lr, C.byref(prm), d_ee2.ptr, d_ns.ptr, d_pass2.ptr, None,
                                              C.byref(counts)))
        return counts

    options = (("composed_lambda_d2h_host_tail_h2d", composed), ("filter_poisson_device", resident))
    for pname, profile in (("baseline_model", 0), ("clean", 1)):
        eng.synth_fill(d_q, n, stride, fixed_len=Lr, seed=2, profile=profile)
        rec = {name: {"step_ms_per_round": []} for name, _ in options}
        for name, fn in options:
            for _ in range(args.warmup):
                fn()
        for _ in range(args.rounds):
            for name, fn in options:
                t = time.perf_counter()
                for _ in range(args.steps):
                    fn()
                rec[name]["step_ms_per_round"].append((time.perf_counter() - t) * 1e3 / args.steps)
        # kernel times in a pass of their own (the event pairs stay out of the step times)
        eng.timing(True)
        for name, fn in options:
            eng.timing_reset()
            for _ in range(5):
                fn()
            kt = eng.kernel_times()
            rec[name]["lambda_kernel_ms"] = kt["lambda"][0] / max(1, kt["lambda"][1])
            if kt["poisson_tail"][1]:
                rec[name]["poisson_tail_kernel_ms"] = kt["poisson_tail"][0] / kt["poisson_tail"][1]
        eng.timing(False)
        composed()
        c = resident()
        ee_i, ps_i = d_ee.download(np.float64, n), d_pass.download(np.uint8, n)
        ee_ii, ps_ii = d_ee2.download(np.float64, n), d_pass2.download(np.uint8, n)
        both = ~(np.isnan(ee_i) | np.isnan(ee_ii)) & (ee_i != 0)
        rel = np.abs(ee_ii[both] - ee_i[both]) / np.abs(ee_i[both])
        rec.update({
            "n_overflow": int(c.n_overflow), "n_pass_resident": int(c.n_pass), "n_pass_composed": int(ps_i.sum()),
            "n_pass_equal": bool(int(c.n_pass) == int(ps_i.sum()) == int(ps_ii.sum())),
            "pass_flags_equal": bool(np.array_equal(ps_i, ps_ii)),
            "nan_equal": bool(np.array_equal(np.isnan(ee_i), np.isnan(ee_ii))),
            "zeros_equal": bool(np.array_equal(ee_i == 0, ee_ii == 0)),
            "worst_relative_difference": float(rel.max()) if rel.size else 0.0,
        })
        for name, _ in options:
            r = rec[name]["step_ms_per_round"]
            rec[name]["step_ms_median"] = float(np.median(r))
            rec[name]["step_ms_spread"] = [float(min(r)), float(max(r))]
        result["profiles"][pname] = rec
        print(pname, json.dumps(rec), flush=True)
    for b in (d_lam, d_ee, d_pass, d_ee2, d_pass2):
        b.free()

    # ---- the host-fed entry, with and without the flag ----
    m = min(args.host_reads, n)
    q = eng.host_alloc((m, stride), np.uint8)
    L.check(lib.mpb_memcpy_d2h(ctx, q.ctypes.data, d_q.ptr, m * stride))               # the clean profile's first m rows
    out = (np.empty(m), np.empty(m, np.int32), np.empty(m, np.uint8))
    host = {"reads": m, "profile": "clean", "reads_per_s": {"host_tail": [], "device_tail": []}}
    for flag in (False, True):
        eng.filter_poisson(q, fixed_len=Lr, out=out, poisson_device_tail=flag)          # warm-up (slots, workspace)
    for _ in range(args.rounds):
        for key, flag in (("host_tail", False), ("device_tail", True)):
            t = time.perf_counter()
            r = eng.filter_poisson(q, fixed_len=Lr, out=out, poisson_device_tail=flag)
            host["reads_per_s"][key].append(m / (time.perf_counter() - t))
            host["n_overflow_" + key] = int(r.n_overflow)
            host["n_pass_" + key] = int(r.n_pass)
    result["host_fed"] = host
    print("host_fed", json.dumps(host), flush=True)

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(result, f, indent=1, sort_keys=True)
    f.write("\n")
print("wrote", args.out)
