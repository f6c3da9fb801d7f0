"""CPU models of the two opt-in arithmetics (MPB_FLAG_FAST_FMA, MPB_FLAG_ODDS; oracle/pb_oracle.c, pbo_filter_batch_model)
without a GPU: pinned bit for bit to an independent pure-Python restatement whose fused multiply-add is exact rational
arithmetic rounded once, their tables pinned to the library's, and the 1e-9 contract (include/moira_pb.h) checked on every
input family tests/test_gpu_opt_in_models.py runs, so that a GPU failure there can only be the kernel's (ODDS_MODE.md)."""
import math
import os
from fractions import Fraction

import numpy as np

import golden_io as G
from helpers import mode_expect as X
from helpers import opt_in_inputs as I

CONTRACT = 1e-9                      # include/moira_pb.h
P0_MIN = 2.0 ** -900
THREADS = max(1, min(16, os.cpu_count() or 1))


def fma(x, y, z):
    """x * y + z rounded once: exact rationals, then one correctly rounded conversion (no libm fma)."""
    return float(Fraction(x) * Fraction(y) + Fraction(z))


def py_tables():
    """{a, b, r} per byte code as the library evaluates them (mpb_hostonly.cpp lut_entry); 0 and 255: the identity {1, 0}."""
    A, B, R = [1.0] * 256, [0.0] * 256, [0.0] * 256
    for c in range(1, 255):
        p = math.pow(10, c / -10.0)
        A[c] = math.pow(1 - p, 1)
        R[c] = p / (1 - p)
        B[c] = (1.0 * R[c]) * A[c]
    return A, B, R


TABLES = py_tables()


def py_model(row, li, arith, alpha, ambigs="treat_as_errors", round_=False, maxerrors=None, uncert=0.01):
    """One read the way the kernels walk it: base by base (ambiguous bases included, as the table's identity step), every
    row at once, then the sequential CDF.  -> (ee after +Ns, rows, p0, hand)."""
    A, B, R = TABLES
    codes = [int(c) for c in row[:li]]
    n_amb = sum(1 for c in codes if c in (0, 255))
    m = li - n_amb
    thr = 1 - alpha
    if m == 0:                       # the oracle's convention for a read without a scored base: ee 0, no row
        e, rows, p0, crossed = 0.0, 0, 1.0, True
    else:
        nrows = m + 2
        v = [1.0] + [0.0] * (nrows - 1)
        p0 = 1.0
        for c in codes:
            a = A[c]
            if arith == "odds":
                for r in range(nrows - 1, 0, -1):
                    v[r] = fma(R[c], v[r - 1], v[r])
                p0 = p0 * a
            else:
                b = B[c]
                for r in range(nrows - 1, 0, -1):
                    v[r] = fma(a, v[r], b * v[r - 1]) if arith == "fma" else a * v[r] + b * v[r - 1]
                v[0] = a * v[0]
        cmp = thr / p0 if arith == "odds" else thr
        acc, js = 0.0, -1
        for j in range(nrows):
            na = acc + v[j]
            if na > cmp:
                js, lo, hi = j, acc, na
                break
            acc = na
        crossed = js >= 0
        rows = js + 1 if crossed else m + 1
        if not crossed:
            e = math.nan
        elif arith == "odds":
            e = (js - 1) + fma(-lo, p0, thr) / (p0 * (hi - lo))
        else:
            e = (js - 1) + (thr - lo) / (hi - lo)
        if e < 0:
            e = 0.0
    if ambigs == "treat_as_errors":
        e = e + n_amb
    hand = not crossed or (arith == "odds" and not p0 >= P0_MIN)
    if not hand and arith != "exact":
        tol = 1e-9 * max(1.0, abs(e))
        limit = maxerrors if maxerrors is not None else li * uncert
        hand = abs(e - limit) <= tol or (round_ and abs(e - round(e)) <= tol)
    return e, rows, p0, hand


def test_models_match_an_exact_rational_restatement(oracle):
    """About 300 short random reads (lengths 0..40, codes 0..255 with extra ambiguous bases), every alpha / ambigs / ROUND
    combination, half of them with maxerrors on one read's own model ee (so that H holds threshold reads): ee, rows, p0 and H
    of the C models equal the restatement's bit for bit.  The restatement's three-rounding twin reproduces the exact oracle."""
    rng = np.random.default_rng(2024)
    n_hand = {"fma": 0, "odds": 0}
    n_reads = 0
    k = 0
    for alpha in (1e-5, 0.005, 0.5, 0.9):
        for ambigs in I.AMBIGS:
            for round_ in (False, True):
                k += 1
                n = 13
                lens = rng.integers(0, 41, n).astype(np.int32)
                q = rng.integers(0, 256, (n, 48)).astype(np.uint8)
                q[rng.random((n, 48)) < 0.06] = 0
                q[rng.random((n, 48)) < 0.06] = 255
                for i in range(n):
                    q[i, lens[i]:] = 0
                n_reads += n
                for arith in ("exact", "fma", "odds"):
                    kw = dict(alpha=alpha, ambigs=ambigs, round_=round_)
                    if k % 2 == 0 and arith != "exact":
                        m0 = oracle.filter_batch_model(q, arith, lens=lens, **kw)
                        fin = np.flatnonzero(np.isfinite(m0.ee_model))
                        kw["maxerrors"] = float(m0.ee_model[fin[len(fin) // 2]])
                    m = oracle.filter_batch_model(q, arith, lens=lens, **kw)
                    for i in range(n):
                        e, rows, p0, hand = py_model(q[i], int(lens[i]), arith, **kw)
                        got = (m.ee_model[i], int(m.rows[i]), m.p0[i], bool(m.hand[i]))
                        assert (e == got[0] or (math.isnan(e) and math.isnan(got[0]))) and (rows, p0, hand) == got[1:], \
                            (arith, kw, i, (e, rows, p0, hand), got)
                    if arith == "exact":
                        ee, ns, ps, rows = oracle.filter_batch(q, lens=lens, **kw)
                        assert X.same(m.ee, ee).all() and np.array_equal(m.rows, rows) and np.array_equal(m.passed, ps.astype(bool))
                        assert np.array_equal(m.ns, ns)
                    else:
                        n_hand[arith] += int((m.hand & np.isfinite(m.ee_model)).sum())
    assert n_reads >= 300
    print("threshold reads in H:", n_hand)
    assert n_hand["fma"] > 0 and n_hand["odds"] > 0


def test_model_tables_are_the_librarys():
    from moira_amd.engine import host_lut
    import pb_oracle
    a, b = host_lut()
    oa, ob = pb_oracle.lut()
    A, B, R = TABLES
    assert np.array_equal(a, oa) and np.array_equal(b, ob)
    assert np.array_equal(a, np.array(A)) and np.array_equal(b, np.array(B))
    for c in range(1, 255):
        assert A[c] * R[c] == B[c], c


def test_odds_range_guard_hands_back_exactly_the_reads_below_2_to_minus_900(oracle):
    s = G.load_set("long_reads")
    q, lens, alpha = s["q"], s["lens"], float(s["alpha"])
    A = np.array(TABLES[0])
    live = np.arange(q.shape[1])[None, :] < lens[:, None]
    log2_p0 = np.where(live, np.log2(A[q]), 0.0).sum(axis=1)
    m = oracle.filter_batch_model(q, "odds", lens=lens, threads=THREADS, alpha=alpha, ambigs="ignore")
    assert np.array_equal(m.hand, log2_p0 < -900) and int(m.hand.sum()) == 6


# ---- the contract on every family of the GPU tests ------------------------------------------------------------------------

def families(oracle):
    """(name, q, lens, fixed_len, [kw, ...]) of every batch tests/test_gpu_opt_in_models.py runs."""
    out = []
    for name, (q, lens, fixed) in (("synth 20k x 300", I.synth300(oracle)), ("ragged 40k x 50-600", I.ragged(oracle))):
        out.append((name, q, lens, fixed, [dict(ambigs=a, round_=r) for a in I.AMBIGS for r in (False, True)]))
    q, lens, fixed = I.wide_class_reads()
    out.append(("wide-class reads", q, lens, fixed, [dict()]))
    for name in G.NPZ_SETS:
        s = G.load_set(name)
        if float(s["alpha"]) >= 1e-5:
            out.append(("set " + name, s["q"], s["lens"], None, [dict(alpha=float(s["alpha"]), ambigs="ignore")]))
    q, lens, fixed = I.synth300(oracle, n=6000, seed=8)
    out.append(("thresholds 6000 x 300", q, lens, fixed, "picks"))
    q, lens, fixed = I.tiny_fraction()
    out.append(("tiny-fraction", q, lens, fixed, [dict(alpha=a, ambigs="ignore", maxerrors=3.0) for a in I.TINY_ALPHAS]))
    q, lens, fixed = I.synth300(oracle, n=6000, seed=4)
    out.append(("alpha sweep 6000 x 300", q, lens, fixed, [dict(alpha=a) for a in I.SWEEP_ALPHAS]))
    q, lens, fixed = I.synth300(oracle, n=20000, seed=3)
    out.append(("flag combinations 20k x 300", q, lens, fixed, [dict()]))
    out.append(("classified 50k x 300",) + I.classified(oracle) + ([dict()],))
    out.append(("host pipeline 600k x 300",) + I.host_pipeline(oracle) + ([dict()],))
    out.append(("clean 2^19 x 300",) + I.clean(oracle) + ([dict()],))
    return out


def threshold_kws(oracle, q, fixed, mode):
    m = oracle.filter_batch_model(q, mode, fixed_len=fixed, threads=THREADS, ambigs="ignore")
    return [dict(maxerrors=me, ambigs="ignore", round_=r) for me in I.threshold_picks(m.ee_model) for r in (False, True)]


def test_the_contract_holds_on_every_gpu_family(oracle):
    """Outside H, each model's ee lies within 1e-9 relative of the exact oracle's and its pass is the oracle's.  Prints, per
    family and mode, the worst relative error and the share of reads whose model result differs from the exact one (the GPU
    tests' "the mode ran" floor is half of it), and for ODDS the share that differs from the FMA model."""
    lines = []
    for name, q, lens, fixed, kws in families(oracle):
        where = dict(fixed_len=fixed) if fixed else dict(lens=lens)
        worst, share, h = {}, {m: [] for m in I.MODES}, {}
        odds_vs_fma = 0.0
        for mode in I.MODES:
            for kw in (threshold_kws(oracle, q, fixed, mode) if kws == "picks" else kws):
                ee, ns, ps, _ = oracle.filter_batch(q, threads=THREADS, **where, **kw)
                m = oracle.filter_batch_model(q, mode, threads=THREADS, **where, **kw)
                keep = ~m.hand
                assert np.array_equal(m.passed[keep], ps[keep].astype(bool)), (name, mode, kw)
                assert np.array_equal(m.ns, ns)
                err = np.abs(m.ee[keep] - ee[keep])
                bound = CONTRACT * np.abs(ee[keep])
                assert np.isfinite(m.ee[keep]).all() and (err <= bound).all(), (name, mode, kw, float((err / np.maximum(np.abs(ee[keep]), 1e-300)).max()))
                rel = float((err / np.where(ee[keep] != 0, np.abs(ee[keep]), 1.0)).max()) if keep.any() else 0.0
                worst[mode] = max(worst.get(mode, 0.0), rel)
                share[mode].append(float(X.differs((ee, ns, ps), m).mean()))
                h[mode] = h.get(mode, 0) + int(m.hand.sum())
                if mode == "odds":
                    f = oracle.filter_batch_model(q, "fma", threads=THREADS, **where, **kw)
                    both = ~m.hand & ~f.hand
                    odds_vs_fma = max(odds_vs_fma, float((both & ~X.same(m.ee, f.ee)).mean()))
        rng = lambda v: "%.0f-%.0f %%" % (100 * min(v), 100 * max(v)) if len(v) > 1 else "%.0f %%" % (100 * v[0])
        line = "%-28s FMA worst %.2g, differs %s | ODDS worst %.2g, differs %s, from FMA %.0f %% | H %d / %d" % (
            name, worst["fma"], rng(share["fma"]), worst["odds"], rng(share["odds"]), 100 * odds_vs_fma, h["fma"], h["odds"])
        print(line)
        lines.append(line)
    assert len(lines) >= 20
