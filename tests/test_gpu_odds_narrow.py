"""MPB_FLAG_ODDS | MPB_FLAG_ODDS_NARROW on the GPU: the natural-order narrow pass in its one-FMA form (k_odds_nar, k_odds_nar_rs,
k_odds_nar_rg; ODDS_MODE.md "The narrow passes"), read by read against the CPU model of the arithmetic (oracle/pb_oracle.c,
pbo_filter_batch_model "odds").  A narrow lane that keeps rows 0 .. R-1 evaluates the model's expressions in the model's order,
so a read the pass finishes has the model's bits; a read it hands back goes through the sorted pipeline with MPB_FLAG_ODDS kept.

The rule for a forced R (check_forced): with F = ~m.hand & ~has_255 & (m.rows <= R) (and the length valid), every read of F equals
the model bit for bit, last_path() says narrow_rows == R and n_fallback == n - |F|, all reads satisfy the counting form
(tests/helpers/mode_expect.py) and the mode is seen to have run over F.  The inputs are tests/helpers/odds_narrow_inputs.py's,
checked on the CPU by tests/test_odds_narrow_inputs.py.  Every call goes through Engine with a resident batch."""
import os

import numpy as np
import pytest

import golden_io as G
from helpers import mode_expect as X
from helpers import odds_narrow_inputs as N
from helpers import opt_in_inputs as I
from helpers.device_runs import Resident
from helpers.odds_forced import check_forced, run          # (the rule for a forced R: shared with test_gpu_narrow_walk.py)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THREADS = N.THREADS


@pytest.fixture(scope="module")
def eng():
    from moira_amd.engine import Engine
    e = Engine(0)
    e.batched_only = True
    yield e
    e.close()


# ---- 1, 2: fixed and ragged shapes ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("R", N.ROWS)
@pytest.mark.parametrize("L,stride", N.FIXED_SHAPES)
def test_fixed_shapes(eng, oracle, L, stride, R):
    q, lens, ex, m, _ = N.reference(oracle, L, stride, False)
    check_forced(eng, q, lens, L, R, ex, m)


@pytest.mark.parametrize("R", N.ROWS)
@pytest.mark.parametrize("L,stride", N.RAGGED_SHAPES)
def test_ragged_shapes_as_they_lie(eng, oracle, L, stride, R):
    q, lens, ex, m, _ = N.reference(oracle, L, stride, True)
    check_forced(eng, q, lens, None, R, ex, m)


@pytest.mark.parametrize("R", N.ROWS)
def test_golden_ragged_set_as_it_lies(eng, oracle, R):
    s = G.load_set("synth_ragged")
    q, lens, alpha = s["q"], s["lens"], float(s["alpha"])
    ex = oracle.filter_batch(q, lens=lens, threads=THREADS, alpha=alpha, ambigs="ignore")[:3]
    m = oracle.filter_batch_model(q, "odds", lens=lens, threads=THREADS, alpha=alpha, ambigs="ignore")
    check_forced(eng, q, lens, None, R, ex, m, mode_ran=False, alpha=alpha, ambigs="ignore")


@pytest.mark.parametrize("R", N.ROWS)
def test_the_references_paired_contigs(eng, oracle, R):
    recs = []
    for kind in ("good", "bad"):
        recs += G.read_fasta_qual(os.path.join(ROOT, "tests", "golden", "reference_test_results", "paired.qc." + kind))
    q, lens = eng.pack([r[2] for r in recs], [r[3] for r in recs], stride=512)
    ex = oracle.filter_batch(q, lens=lens, threads=THREADS)[:3]
    m = oracle.filter_batch_model(q, "odds", lens=lens, threads=THREADS)
    check_forced(eng, q, lens, None, R, ex, m, mode_ran=False)


def test_lengths_outside_the_row_fail_the_call_as_without_the_flag(eng, oracle):
    q, lens, ex, m, _ = N.reference(oracle, 300, 320, True)
    lens = lens.copy()
    lens[[5, 700]] = (-1, 321)
    errs = []
    for kw in (dict(narrow_rows=2), dict(odds=True, odds_narrow=True, narrow_rows=2)):
        with pytest.raises(ValueError, match="2 read length") as e:
            run(eng, q, lens, None, **kw)
        errs.append(str(e.value))
    assert errs[0] == errs[1]
    run(eng, q, N.reference(oracle, 300, 320, True)[1], None, no_narrow=True)        # (a clean call: the counter is reported once)


# ---- 3: partial blocks --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("n", N.PARTIAL_N)
def test_partial_blocks(eng, oracle, n, ragged):
    if ragged:
        q, lens = oracle.synth_fill(n, 640, min_len=50, max_len=600, seed=5 + n, profile=1)
        w, fixed = dict(lens=lens), None
    else:
        q, lens = oracle.synth_fill(n, 320, fixed_len=300, seed=5 + n, profile=1)
        w, fixed = dict(fixed_len=300), 300
    ex = oracle.filter_batch(q, threads=4, **w)[:3]
    m = oracle.filter_batch_model(q, "odds", threads=4, **w)
    check_forced(eng, q, lens, fixed, 2, ex, m, mode_ran=n >= 255)


# ---- 4: modes -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("stride", N.MODE_STRIDES)
@pytest.mark.parametrize("kw", N.MODE_KW, ids=lambda kw: "-".join("%s=%s" % i for i in kw.items()))
def test_modes(eng, oracle, kw, stride):
    q, lens, fixed = N.modes_batch(oracle, stride)
    ex = oracle.filter_batch(q, fixed_len=fixed, threads=THREADS, **kw)[:3]
    m = oracle.filter_batch_model(q, "odds", fixed_len=fixed, threads=THREADS, **kw)
    for R in N.ROWS:
        done, _ = check_forced(eng, q, lens, fixed, R, ex, m, **kw)
        if kw.get("alpha") == 1e-4:
            assert (done > 0) == (R >= 3)
        if kw.get("alpha") == 1e-5:
            assert (done > 0) == (R == 4)


# ---- 5: the decision guard ----------------------------------------------------------------------------------------------------------

def test_decision_guard(eng, oracle):
    q, lens, fixed = I.synth300(oracle, n=6000, seed=8)
    m0 = oracle.filter_batch_model(q, "odds", fixed_len=fixed, threads=THREADS, ambigs="ignore")
    picks = I.threshold_picks(m0.ee_model)
    assert len(picks) >= 5
    for me in picks:
        for round_ in (False, True):
            kw = dict(maxerrors=me, ambigs="ignore", round_=round_)
            ex = oracle.filter_batch(q, fixed_len=fixed, threads=THREADS, **kw)
            m = oracle.filter_batch_model(q, "odds", fixed_len=fixed, threads=THREADS, **kw)
            assert m.hand.sum() >= 1
            _, novf = check_forced(eng, q, lens, fixed, 4, ex[:3], m, mode_ran=not round_, **kw)
            # a read of H that the sorted pipeline's class holds reaches the overflow pass through k_dp_odds' own guard; one whose
            # class is too narrow (a budget miss) is counted there as well -- so at least the former
            assert novf >= int((m.hand & (m.rows <= ex[3])).sum()), (me, round_, novf)


# ---- 6: the reference's vector sets ---------------------------------------------------------------------------------------------------

def reference_exact(s):
    ee = G.expected_value(s)
    with np.errstate(invalid="ignore"):
        ps = ee <= s["lens"] * 0.01
    return ee, s["ns_ref"].astype(np.int32), ps


@pytest.mark.parametrize("name", G.NPZ_SETS)
def test_reference_vector_sets(eng, oracle, name):
    s = G.load_set(name)
    q, lens, alpha = s["q"], s["lens"], float(s["alpha"])
    kw = dict(alpha=alpha, ambigs="ignore")
    if alpha < 1e-5:
        with pytest.raises(ValueError, match="needs alpha >= 1e-5"):
            run(eng, q, lens, None, odds=True, odds_narrow=True, narrow_rows=2, **kw)
        return
    ex = reference_exact(s)
    m = oracle.filter_batch_model(q, "odds", lens=lens, threads=THREADS, **kw)
    for R in (2, 4):
        # as they lie: one ragged batch (rows wider than the pass takes go through the sorted pipeline)
        got, c, path = run(eng, q, lens, None, odds=True, odds_narrow=True, narrow_rows=R, **kw)
        assert path["narrow_rows"] == (R if q.shape[1] <= 4096 else 0)
        X.check_counting_form(got, ex, m, c.n_overflow, n_wide=int((m.rows > 1024).sum()))
        if name == "long_reads":
            continue
        # regrouped by length: fixed-length batches
        for L in np.unique(lens):
            if L < 1:
                continue
            idx = np.flatnonzero(lens == L)
            sub = I_sub(m, idx)
            got, c, path = run(eng, q[idx], lens[idx], int(L), odds=True, odds_narrow=True, narrow_rows=R, **kw)
            assert path["narrow_rows"] == R
            X.check_counting_form(got, tuple(a[idx] for a in ex), sub, c.n_overflow)
            F = N.finished(sub, q[idx], lens[idx], R)
            assert X.matches(*got, sub.ee, ex[1][idx], sub.passed)[F].all(), (name, int(L), R)
            assert path["n_fallback"] == len(idx) - int(F.sum())


def I_sub(m, sel):
    import pb_oracle
    return pb_oracle.ModelResult(**{k: v[sel] for k, v in m.__dict__.items()})


# ---- 7: the choice ------------------------------------------------------------------------------------------------------------------

def test_the_choice(eng, oracle):
    q, lens, fixed = I.clean(oracle)
    n = len(q)
    ex = oracle.filter_batch(q, fixed_len=fixed, threads=THREADS)[:3]
    m = oracle.filter_batch_model(q, "odds", fixed_len=fixed, threads=THREADS)
    res = Resident(eng, q)
    try:
        ee, ns, ps, c, path, _ = res.run(fixed_len=fixed, odds=True, odds_narrow=True)
        R = path["narrow_rows"]
        assert path["sampled"] and R >= 2, path
        F = N.finished(m, q, lens, R)
        assert path["n_fallback"] == n - int(F.sum())
        assert X.matches(ee, ns, ps, m.ee, ex[1], m.passed)[F].all()
        X.check_counting_form((ee, ns, ps), ex, m, c.n_overflow)
        X.check_mode_ran((ee, ns, ps), ex, m, among=F)
        # a second call of the same shape is not sampled
        _, _, _, _, path, _ = res.run(fixed_len=fixed, odds=True, odds_narrow=True)
        assert not path["sampled"] and path["narrow_rows"] == R
        # odds alone: the sorted pipeline
        ee, ns, ps, c, path, _ = res.run(fixed_len=fixed, odds=True)
        assert path["narrow_rows"] == 0
        X.check_counting_form((ee, ns, ps), ex, m, c.n_overflow)
        # BASELINE's model in the same buffer after the clean batch: the cached choice hands everything back
        res.run(fixed_len=fixed, odds=True, odds_narrow=True)
        qb, _ = oracle.synth_fill(n, q.shape[1], fixed_len=fixed, seed=41, profile=0)
        res.d_q.upload(np.ascontiguousarray(qb).reshape(-1))
        exb = oracle.filter_batch(qb, fixed_len=fixed, threads=THREADS)[:3]
        mb = oracle.filter_batch_model(qb, "odds", fixed_len=fixed, threads=THREADS)
        ee, ns, ps, c, path, _ = res.run(fixed_len=fixed, odds=True, odds_narrow=True)
        assert not path["sampled"] and path["narrow_rows"] == R and path["n_fallback"] == n, path
        X.check_counting_form((ee, ns, ps), exb, mb, c.n_overflow)
        _, _, _, _, path, _ = res.run(fixed_len=fixed, odds=True, odds_narrow=True)
        assert path["sampled"]
    finally:
        res.free()


# ---- 8: what keeps the flag out -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flag", ["no_narrow", "decision_only", "count_cells", "test_underpredict"])
def test_what_keeps_a_call_out_of_the_pass(eng, oracle, flag):
    q, lens, fixed = N.modes_batch(oracle, 320)
    ee0, ns0, ps0, _ = oracle.filter_batch(q, fixed_len=fixed, threads=THREADS)
    (ee, ns, ps), c, path = run(eng, q, lens, fixed, odds=True, odds_narrow=True, narrow_rows=2, **{flag: True})
    assert path["narrow_rows"] == 0
    assert np.array_equal(ps.astype(bool), ps0.astype(bool)) and np.array_equal(ns, ns0)
    live = np.isfinite(ee)                                             # (decision_only settles reads at +inf)
    assert np.array_equal(np.isnan(ee), np.isnan(ee0))
    fin = live & np.isfinite(ee0) & (ee0 > 0)
    assert (np.abs(ee[fin] - ee0[fin]) <= 1e-9 * ee0[fin]).all() and (ee[live & (ee0 == 0)] == 0).all()


def test_a_private_table_keeps_the_call_out_of_the_pass(eng, oracle):
    """Scores above 254: the call runs on a private table, which has no odds twin -- exact results throughout, as with
    MPB_FLAG_ODDS alone (tests/test_gpu_odds.py).  (The host entry that carries such a table never takes the narrow pass.)"""
    rng = np.random.default_rng(3)
    seqs = ["".join(rng.choice(list("ACGT"), 120)) for _ in range(6000)]
    quals = [[int(v) for v in rng.integers(30, 41, 120)] for _ in range(6000)]
    for k in range(0, 6000, 7):
        quals[k][5] = 300
    q, lens, codes = eng.pack_coded(seqs, quals)
    r0 = eng.filter(q, lens=lens, code_scores=codes)
    r = eng.filter(q, lens=lens, code_scores=codes, odds=True, odds_narrow=True, narrow_rows=2)
    assert np.array_equal(r.ee, r0.ee, equal_nan=True) and np.array_equal(r.passed, r0.passed) and np.array_equal(r.ns, r0.ns)


def test_the_flag_alone_is_refused(eng, oracle):
    from moira_amd import _lib as L
    q, lens, ex, m, _ = N.reference(oracle, 100, 112, False)
    res = Resident(eng, q)
    try:
        prm = eng.params()
        prm.flags |= L.FLAG_ODDS_NARROW
        qp, ee, ns, ps = res.ptrs()
        with pytest.raises(ValueError, match="needs MPB_FLAG_ODDS"):
            eng.filter_device(qp, res.n, res.stride, fixed_len=100, d_ee=ee, d_ns=ns, d_pass=ps, params=prm)
    finally:
        res.free()
