"""MPB_FLAG_FAST_FMA and MPB_FLAG_ODDS on the GPU, read by read against the CPU models of their arithmetic
(oracle/pb_oracle.c, pbo_filter_batch_model): each read equals the model bit for bit, or the exact oracle where the mode's
own rules hand it to the three-rounding pass (tests/helpers/mode_expect.py states both forms of the rule).  Every input
family here is checked on the CPU to lie within the 1e-9 contract (tests/test_opt_in_models.py), so a failure is the kernel's.
Every call goes through Engine (ctypes -> the built library)."""
import numpy as np
import pytest

import golden_io as G
from helpers import mode_expect as X
from helpers import opt_in_inputs as I

pytestmark = pytest.mark.gpu

THREADS = 16


@pytest.fixture(scope="module")
def eng():
    from moira_amd.engine import Engine
    e = Engine(0)
    e.batched_only = True
    yield e
    e.close()


def where(lens, fixed):
    return dict(fixed_len=fixed) if fixed else dict(lens=lens)


def device_run(eng, q, lens, fixed, params, budgets=True):
    """One resident batch through mpb_filter_device -> ((ee, ns, pass), budgets or None, counts)."""
    n, stride = q.shape
    d_q = eng.alloc(q.nbytes).upload(q)
    d_len = eng.alloc(n * 4).upload(np.ascontiguousarray(lens, np.int32)) if not fixed else None
    d_ee, d_ns, d_pass = eng.alloc(n * 8), eng.alloc(n * 4), eng.alloc(n)
    c = eng.filter_device(d_q, n, stride, d_len=d_len, fixed_len=fixed or 0, d_ee=d_ee, d_ns=d_ns, d_pass=d_pass, params=params)
    got = (d_ee.download(np.float64, n), d_ns.download(np.int32, n), d_pass.download(np.uint8, n))
    budgets = eng.read_budgets(n) if budgets else None
    for b in (d_q, d_len, d_ee, d_ns, d_pass):
        if b is not None:
            b.free()
    return got, budgets, c


def exact_form(eng, oracle, mode, tag, q, lens, fixed, exact=None, settled_ok=False, **kw):
    """The per-read rule, exact form, on one resident batch; the mode-ran floor.  -> (got, budgets, model, exact)."""
    w = where(lens, fixed)
    flags = {k: kw.pop(k) for k in ("decision_only", "test_underpredict", "count_cells") if k in kw}
    ex = exact if exact is not None else oracle.filter_batch(q, threads=THREADS, **w, **kw)[:3]
    m = oracle.filter_batch_model(q, mode, threads=THREADS, **w, **kw)
    got, budgets, c = device_run(eng, q, lens, fixed, eng.params(**kw, **flags, **I.mode_kw(mode)))
    settled = np.zeros(len(q), bool)
    if settled_ok:
        settled = np.isinf(got[0])
        assert settled.any()
        assert (budgets[settled] == 0).all() and not got[2][settled].any() and not np.asarray(ex[2])[settled].any()
        assert np.array_equal(got[1][settled], np.asarray(ex[1])[settled])
    h, miss, _ = X.check_exact_form(got, ex, m, budgets, c.n_overflow, settled=settled)
    live = ~settled
    gpu, cpu = X.check_mode_ran(got, ex, m, among=live & ~X.expect(ex, m, budgets)["must_exact"])
    print("[%s] %s: |H| %d, budget misses predicted %d, n_overflow %d, k_wide %d%s, model != exact %.1f %% (GPU %.1f %%)" % (
        mode, tag, h, miss, c.n_overflow, int(((budgets == 0) & live).sum()),
        ", settled %d" % int(settled.sum()) if settled_ok else "", 100 * cpu, 100 * gpu))
    if flags.get("test_underpredict"):
        assert miss > 1000
    return got, budgets, m, ex


def sub_model(m, sel):
    import pb_oracle
    return pb_oracle.ModelResult(**{k: v[sel] for k, v in m.__dict__.items()})


# ---- synthetic batches ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", I.MODES)
@pytest.mark.parametrize("family", ["synth300", "ragged"])
def test_synthetic_batches(eng, oracle, mode, family):
    q, lens, fixed = getattr(I, family)(oracle)
    for ambigs in I.AMBIGS:
        for round_ in (False, True):
            exact_form(eng, oracle, mode, "%s %s round=%s" % (family, ambigs, round_), q, lens, fixed, ambigs=ambigs, round_=round_)


# ---- long reads -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", I.MODES)
def test_long_reads(eng, oracle, mode):
    q, lens, fixed = I.wide_class_reads()
    _, budgets, _, _ = exact_form(eng, oracle, mode, "wide-class reads", q, lens, fixed)
    assert budgets.max() >= 512
    s = G.load_set("long_reads")
    alpha = float(s["alpha"])
    exact = reference_exact(s)
    _, budgets, m, _ = exact_form(eng, oracle, mode, "long_reads.npz", s["q"], s["lens"], None, exact=exact, alpha=alpha, ambigs="ignore")
    assert (budgets == 0).sum() >= 1                                   # k_wide ran
    if mode == "odds":
        assert int((m.hand & (budgets > 0)).sum()) >= 1               # the range guard handed reads back


# ---- the reference's vector sets ----------------------------------------------------------------------------------------------

def reference_exact(s):
    """(ee, ns, pass) from the reference's own values (ambigs ignore, default uncert 0.01)."""
    ee = G.expected_value(s)
    with np.errstate(invalid="ignore"):
        ps = ee <= s["lens"] * 0.01
    return ee, s["ns_ref"].astype(np.int32), ps


@pytest.mark.parametrize("mode", I.MODES)
@pytest.mark.parametrize("name", G.NPZ_SETS)
def test_reference_vector_sets(eng, oracle, mode, name):
    s = G.load_set(name)
    alpha = float(s["alpha"])
    if alpha < 1e-5:
        with pytest.raises(ValueError, match="needs alpha >= 1e-5"):
            eng.filter(s["q"], lens=s["lens"], alpha=alpha, ambigs="ignore", **I.mode_kw(mode))
        return
    exact_form(eng, oracle, mode, "set " + name, s["q"], s["lens"], None, exact=reference_exact(s), alpha=alpha, ambigs="ignore")


# ---- thresholds on reads' own values, tiny fractions, the alpha sweep ---------------------------------------------------------

@pytest.mark.parametrize("mode", I.MODES)
def test_thresholds_on_reads_own_values(eng, oracle, mode):
    q, lens, fixed = I.synth300(oracle, n=6000, seed=8)
    m0 = oracle.filter_batch_model(q, mode, fixed_len=fixed, threads=THREADS, ambigs="ignore")
    picks = I.threshold_picks(m0.ee_model)
    assert len(picks) >= 5
    for me in picks:
        for round_ in (False, True):
            _, budgets, m, _ = exact_form(eng, oracle, mode, "maxerrors %r round=%s" % (me, round_), q, lens, fixed,
                                          maxerrors=me, ambigs="ignore", round_=round_)
            assert m.hand.sum() >= 1


@pytest.mark.parametrize("mode", I.MODES)
def test_tiny_fraction_batch(eng, oracle, mode):
    q, lens, fixed = I.tiny_fraction()
    for alpha in I.TINY_ALPHAS:
        exact_form(eng, oracle, mode, "tiny-fraction alpha %g" % alpha, q, lens, fixed, alpha=alpha, ambigs="ignore", maxerrors=3.0)


@pytest.mark.parametrize("mode", I.MODES)
def test_alpha_sweep(eng, oracle, mode):
    q, lens, fixed = I.synth300(oracle, n=6000, seed=4)
    for alpha in I.SWEEP_ALPHAS:
        exact_form(eng, oracle, mode, "alpha %g" % alpha, q, lens, fixed, alpha=alpha)


# ---- FAST_FMA on the one-read path (k_small<true>) -----------------------------------------------------------------------------

def launches(eng, fn):
    eng.timing(True)
    eng.timing_reset()
    try:
        r = fn()
        kt = eng.kernel_times()
    finally:
        eng.timing(False)
    return r, {k: v[1] for k, v in kt.items()}


def test_fast_fma_on_the_one_read_path(eng, oracle):
    q, lens, fixed = I.synth300(oracle, n=60000, seed=4)
    ex = oracle.filter_batch(q, fixed_len=fixed, threads=THREADS)[:3]
    m = oracle.filter_batch_model(q, "fma", fixed_len=fixed, threads=THREADS)
    _, budgets, _ = device_run(eng, q, lens, fixed, eng.params(fast_fma=True))
    caps = sorted(eng.class_histogram())
    below = {c: max([x for x in caps if x < c], default=1) for c in caps}
    # reads whose model rows fit the cap BELOW their class: the prediction lies above that cap, so the one-read path's class
    # (the next power of two at or above the prediction) holds them too -- no budget miss sends the batch down the pipeline
    fits = np.flatnonzero(~m.hand & (budgets > 0) & (m.rows <= np.array([below.get(int(b), 0) for b in budgets])))
    assert len(fits) >= 4096
    for n in (1, 64, 4096):
        sel = fits[:n]
        r, k = launches(eng, lambda: eng.filter(q[sel], fixed_len=fixed, fast_fma=True, batched_only=False))
        assert k["prepass"] == 0 and k["dp"] >= 1, k                       # k_small alone: no prepass, no sort
        got = (r.ee, r.ns, r.passed)
        sm, sx = sub_model(m, sel), tuple(np.asarray(a)[sel] for a in ex)
        ok = X.matches(*got, sm.ee, sx[1], sm.passed)
        assert ok.all(), (n, np.flatnonzero(~ok)[:5].tolist())
        gpu, cpu = X.check_mode_ran(got, sx, sm)
        print("[fma] one-read path, %d reads: every read equals the model, model != exact %.1f %% (GPU %.1f %%)" % (n, 100 * cpu, 100 * gpu))
    # one read of H in the batch: k_small<true> reports pass = 2 and the batch goes down the pipeline
    sel = fits[:64]
    me = float(m.ee_model[sel[7]])
    mh = oracle.filter_batch_model(q[sel], "fma", fixed_len=fixed, threads=THREADS, maxerrors=me)
    eh = oracle.filter_batch(q[sel], fixed_len=fixed, threads=THREADS, maxerrors=me)[:3]
    assert mh.hand[7] and mh.hand.sum() >= 1
    r, k = launches(eng, lambda: eng.filter(q[sel], fixed_len=fixed, fast_fma=True, batched_only=False, maxerrors=me))
    assert k["prepass"] >= 1, k
    off = X.check_counting_form((r.ee, r.ns, r.passed), eh, mh, r.n_overflow)
    print("[fma] one-read path with a read of H: |H| %d, n_overflow %d, reads off the model %d" % (int(mh.hand.sum()), r.n_overflow, off))


# ---- entries: classified at source, the host pipeline ----------------------------------------------------------------------

@pytest.mark.parametrize("mode", I.MODES)
def test_classified_entry(eng, oracle, mode):
    q, lens, L = I.classified(oracle)
    n, stride = q.shape
    ex = oracle.filter_batch(q, fixed_len=L, threads=THREADS)[:3]
    m = oracle.filter_batch_model(q, mode, fixed_len=L, threads=THREADS)
    d_q = eng.alloc(n * stride).upload(q)
    d_seq, d_qual, d_out = eng.alloc(n * stride), eng.alloc(n * stride), eng.alloc(n * stride)
    d_ee, d_ns, d_pass = eng.alloc(n * 8), eng.alloc(n * 4), eng.alloc(n)
    eng.encode_ascii_device(d_q, n, stride, d_seq, d_qual)
    c = eng.filter_ascii_device(d_seq, d_qual, n, stride, d_out, fixed_len=L, d_ee=d_ee, d_ns=d_ns, d_pass=d_pass,
                                params=eng.params(**I.mode_kw(mode)))
    got = (d_ee.download(np.float64, n), d_ns.download(np.int32, n), d_pass.download(np.uint8, n))
    for b in (d_q, d_seq, d_qual, d_out, d_ee, d_ns, d_pass):
        b.free()
    off = X.check_counting_form(got, ex, m, c.n_overflow)
    gpu, cpu = X.check_mode_ran(got, ex, m)
    print("[%s] classified 50k x 300: |H| %d, n_overflow %d, reads off the model %d, model != exact %.1f %% (GPU %.1f %%)" % (
        mode, int(m.hand.sum()), c.n_overflow, off, 100 * cpu, 100 * gpu))


@pytest.mark.parametrize("mode", I.MODES)
def test_host_pipeline_in_chunks(eng, oracle, mode):
    q, lens, fixed = I.host_pipeline(oracle)
    assert q.nbytes >= 192 * 10 ** 6
    ex = oracle.filter_batch(q, fixed_len=fixed, threads=THREADS)[:3]
    m = oracle.filter_batch_model(q, mode, fixed_len=fixed, threads=THREADS)
    r, k = launches(eng, lambda: eng.filter(q, fixed_len=fixed, **I.mode_kw(mode)))
    assert k["prepass"] >= 2, k                                            # at least two chunks
    got = (r.ee, r.ns, r.passed)
    off = X.check_counting_form(got, ex, m, r.n_overflow)
    gpu, cpu = X.check_mode_ran(got, ex, m)
    print("[%s] host pipeline 600k x 300 (%d chunks): |H| %d, n_overflow %d, reads off the model %d, model != exact %.1f %% "
          "(GPU %.1f %%)" % (mode, k["prepass"], int(m.hand.sum()), r.n_overflow, off, 100 * cpu, 100 * gpu))


# ---- flag combinations ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", I.MODES)
def test_flag_combinations(eng, oracle, mode):
    q, lens, fixed = I.synth300(oracle, n=20000, seed=3)
    ex = oracle.filter_batch(q, fixed_len=fixed, threads=THREADS)[:3]
    exact_form(eng, oracle, mode, "decision_only", q, lens, fixed, exact=ex, settled_ok=True, decision_only=True)
    exact_form(eng, oracle, mode, "test_underpredict", q, lens, fixed, exact=ex, test_underpredict=True)     # > 1000 misses
    plain, _, _, _ = exact_form(eng, oracle, mode, "plain", q, lens, fixed, exact=ex)
    counted, _, _, _ = exact_form(eng, oracle, mode, "count_cells", q, lens, fixed, exact=ex, count_cells=True)
    assert all(np.array_equal(a, b) for a, b in zip(plain, counted))


@pytest.mark.parametrize("mode", I.MODES)
def test_the_mode_keeps_a_clean_batch_out_of_the_narrow_pass(eng, oracle, mode):
    q, lens, fixed = I.clean(oracle)
    device_run(eng, q, lens, fixed, eng.params(), budgets=False)
    assert eng.last_path()["narrow_rows"] >= 2
    exact_form(eng, oracle, mode, "clean 2^19", q, lens, fixed)
    assert eng.last_path()["narrow_rows"] == 0
