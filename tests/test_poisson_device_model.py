"""The device tail of --error_calc poisson, without a GPU: the numpy model of k_poisson_tail (tests/helpers/poisson_tail_model.py --
recurrence, window, mode_unsure, hand-back mask) with em = exp(-lambda) at -1 / 0 / +1 ulp against mpb_poisson_finish_host, over
every input family tests/test_gpu_poisson_device.py uses.  This is where the window of rule (b) was fixed: the worst relative
error the test prints per alpha is what include/moira_pb.h and DESIGN.md quote."""
import numpy as np
import pytest

import golden_io as G
from helpers import poisson_tail_model as P
from moira_amd import _lib as L

MARGIN = 10          # the model's worst case must lie at least this far inside the contract


def check(lam, ns, lens, worst, share=None, planted=0, **kw):
    """One family at one setting, em at -1 / 0 / +1 ulp -> the reads rules (b) and (c) hand back (the largest count of the three)."""
    raw, _ = P.host_tail(lam, ns, lens, alpha=kw["alpha"], ambigs="ignore")
    hee, hps = P.host_tail(lam, ns, lens, **kw)
    with np.errstate(invalid="ignore"):
        in_range = (lam >= 0) & (lam <= P.LAMBDA_MAX)
    assert not np.isnan(raw[in_range]).any()                    # no read with lambda <= 64 (alpha >= 1e-5) is NaN on the host
    most = 0
    for ulp in (-1, 0, 1):
        m = P.model(lam, ns, lens, ulp=ulp, **kw)
        kept = ~m["back"]
        assert np.array_equal(m["a"], ~in_range) and not (kept & ~in_range).any()
        assert P.close(m["ee"][kept], m["ps"][kept], hee[kept], hps[kept]).all(), (kw, ulp)
        assert np.array_equal(m["j"][kept], P.host_cross_term(raw)[kept]), (kw, ulp)      # the crossing term never differs
        err = P.rel_err(m["ee"][kept], hee[kept])
        if err.size:
            worst[kw["alpha"]] = max(worst.get(kw["alpha"], 0.0), float(err.max()))
        most = max(most, int((m["b"] | m["c"]).sum()))
    if share is not None:
        assert most - planted <= share * len(lam), (kw, most)
    return most


def report(worst, what):
    print("\n[poisson device tail model] %s, window 2^%d: worst relative error per alpha: %s"
          % (what, int(np.log2(P.WINDOW)), ", ".join("%g: %.2e" % (a, worst[a]) for a in sorted(worst))))
    assert worst and max(worst.values()) * MARGIN <= P.CONTRACT, worst


def test_model_on_the_lambda_grid():
    worst = {}
    for alpha in P.MODEL_ALPHAS:
        g = P.lambda_grid(alpha)
        fixed = np.full(P.GRID_N, 300, np.int32)
        for kw in P.settings((alpha,)):
            for lens in (g["lens"], fixed):
                check(g["lam"], g["ns"], lens, worst, share=P.CAP_SHARE, planted=g["n_planted"], **kw)
    report(worst, "lambda grid")


def test_model_on_uniform_lambdas_100k():
    """The measurement the window was chosen on: 100 k lambda uniform in [0, 64], six alpha."""
    rng = np.random.default_rng(5)
    lam = rng.uniform(0, 64, 100_000)
    ns, lens = np.zeros(len(lam), np.int32), np.full(len(lam), 300, np.int32)
    worst = {}
    for alpha in P.MODEL_ALPHAS:
        check(lam, ns, lens, worst, share=P.CAP_SHARE, alpha=alpha, ambigs="ignore")
    report(worst, "100 k uniform lambda")


def test_model_on_the_limit_family():
    f = P.limit_family()
    worst = {}
    hee, _ = P.host_tail(f["lam"], f["ns"], f["lens"], alpha=0.005)
    picks = [k for k in range(len(hee)) if hee[k] > 0.5][:6]
    for k in picks:
        kw = dict(alpha=0.005, maxerrors=float(hee[k]))
        check(f["lam"], f["ns"], f["lens"], worst, share=P.CAP_SHARE, planted=1, **kw)
        for ulp in (-1, 0, 1):
            assert P.model(f["lam"], f["ns"], f["lens"], ulp=ulp, **kw)["c"][k]              # the read on the limit is handed back
    lam = np.concatenate([P.integer_lambdas(), f["lam"][:994]])
    for ambigs in P.AMBIGS:
        kw = dict(alpha=0.005, round_=True, ambigs=ambigs)
        check(lam, f["ns"], f["lens"], worst, share=P.CAP_SHARE, planted=6, **kw)
        for ulp in (-1, 0, 1):
            assert P.model(lam, f["ns"], f["lens"], ulp=ulp, **kw)["c"][:6].all()
    report(worst, "limit family")


@pytest.mark.parametrize("stride", P.MATRIX_STRIDES)
def test_model_on_the_matrix_families(stride):
    q, lens, full = P.matrix_family(stride)
    worst = {}
    for mat, ll in ((q, lens), (full, None)):
        lam, ns = P.lambda_of(mat, ll)
        ll = np.full(len(lam), stride, np.int32) if ll is None else ll
        for kw in (dict(alpha=0.005), dict(alpha=1e-5, ambigs="ignore"), dict(alpha=0.05, round_=True)):
            # (no cap here, as in the GPU test: a one-base read of Q48..Q56 has a lambda inside the window of alpha = 1e-5)
            check(lam, ns, ll, worst, **kw)
    report(worst, "matrix family, stride %d" % stride)


def test_model_hands_back_everything_outside_the_range():
    for q, fixed in P.handed_back_family():
        lam, ns = P.lambda_of(q)
        m = P.model(lam, ns, np.full(len(lam), fixed), alpha=0.005)
        assert m["a"].all() and (m["ps"] == 2).all() and np.array_equal(m["ee"], lam)
    hee, _ = P.host_tail(P.lambda_of(P.handed_back_family()[0][0])[0], np.zeros(300), np.full(300, 1024), alpha=0.005)
    assert np.isfinite(hee).all()
    hee, _ = P.host_tail(P.lambda_of(P.handed_back_family()[1][0])[0], np.zeros(300), np.full(300, 2048), alpha=0.005)
    assert np.isnan(hee).all()


def test_model_on_the_reference_set():
    z = G.load_set("poisson")
    worst, seen = {}, 0
    for t in ("a", "b"):
        lam, ns = P.lambda_of(z["q_" + t], z["lens_" + t])
        for ai, alpha in enumerate(z["alphas"]):
            if alpha < 1e-5:
                continue
            seen += 1
            check(lam, ns, z["lens_" + t], worst, alpha=float(alpha), ambigs="ignore")
            m = P.model(lam, ns, z["lens_" + t], alpha=float(alpha), ambigs="ignore")
            o = z["ovf_" + t][ai].astype(bool)
            assert m["a"][o].all()                                          # every read the reference overflowed on is handed back
            kept = ~m["back"]
            assert (P.rel_err(m["ee"][kept], z["ee_" + t][ai][kept]) <= P.CONTRACT / MARGIN).all()
    assert seen >= 2
    report(worst, "reference set")


def test_model_on_the_pipeline_batch(oracle):
    n = 300_017
    q, lens = oracle.synth_fill(n, 608, min_len=50, max_len=600, seed=5)
    lam, ns = P.lambda_of(q, lens)
    worst = {}
    most = check(lam, ns, lens, worst, alpha=0.005, ambigs="treat_as_errors")
    assert most <= P.CAP_SHARE * n
    report(worst, "pipeline batch")


def test_flag_and_prototypes_are_declared():
    assert L.FLAG_POISSON_DEVICE_TAIL == 1 << 21 and L.KERNEL_NAMES[10] == "poisson_tail"
    lib = L.load()
    assert hasattr(lib, "mpb_poisson_finish_device") and hasattr(lib, "mpb_filter_poisson_device")
    from moira_amd.engine import Engine
    assert Engine.params(poisson_device_tail=True).flags & L.FLAG_POISSON_DEVICE_TAIL
    assert not Engine.params().flags & L.FLAG_POISSON_DEVICE_TAIL
