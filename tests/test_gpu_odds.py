"""MPB_FLAG_ODDS on the GPU (ODDS_MODE.md, include/moira_pb.h): ee within 1e-9 relative of the bit-exact result, ns, pass and the
NaN pattern identical -- and the mode really runs: a tolerance test passes trivially if every read is recomputed exactly, so
the reads handed to the three-rounding pass are counted (n_overflow) against what the two guards may hand over.
Every call goes through Engine (ctypes -> the built library)."""
import numpy as np
import pytest

import golden_io as G
from helpers import odds_model as M

pytestmark = pytest.mark.gpu

REL_TOL = 1e-9      # the contract


@pytest.fixture(scope="module")
def eng():
    from moira_amd.engine import Engine
    e = Engine(0)
    e.batched_only = True
    yield e
    e.close()


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def worst_rel(got, want):
    assert np.array_equal(np.isnan(got), np.isnan(want))
    fin = np.isfinite(want) & (want != 0)
    assert same(got[~fin], want[~fin])
    return float((np.abs(got[fin] - want[fin]) / np.abs(want[fin])).max()) if fin.any() else 0.0


def log2_p0(q, lens):
    a, _ = M.tables()
    live = np.arange(q.shape[1])[None, :] < np.asarray(lens)[:, None]
    return np.where(live, np.log2(a[q]), 0.0).sum(axis=1)


BATCHES = [dict(n=20000, stride=320, fixed_len=300, seed=4), dict(n=40000, stride=608, min_len=50, max_len=600, seed=5)]


@pytest.mark.parametrize("which", [0, 1])
def test_tolerance_decisions_and_the_mode_really_ran(eng, oracle, which):
    b = dict(BATCHES[which])
    n, stride = b.pop("n"), b.pop("stride")
    q, lens = oracle.synth_fill(n, stride, **b)
    fixed = b.get("fixed_len")
    where = dict(fixed_len=fixed) if fixed else dict(lens=lens)
    lens_all = np.full(n, fixed) if fixed else lens
    guarded_by_range = int((log2_p0(q, lens_all) < -899).sum())
    for ambigs in ("treat_as_errors", "ignore", "disallow"):
        plain, _, _, _ = oracle.filter_batch(q, threads=8, ambigs=ambigs, **where)
        limit = lens_all * 0.01                                               # default thresholds: uncert 0.01
        near_limit = np.abs(plain - limit) <= 1e-8 * np.maximum(1.0, np.abs(plain))
        near_int = np.abs(plain - np.rint(plain)) <= 1e-8 * np.maximum(1.0, np.abs(plain))
        for round_ in (False, True):
            kw = dict(ambigs=ambigs, round_=round_)
            ee, ns, ps, _ = oracle.filter_batch(q, threads=8, **kw, **where)
            r0 = eng.filter(q, **where, **kw)
            r = eng.filter(q, odds=True, **where, **kw)
            assert same(r0.ee, ee)
            rel = worst_rel(r.ee, ee)
            allowed = guarded_by_range + int(near_limit.sum()) + (int((near_int & ~near_limit).sum()) if round_ else 0)
            extra = r.n_overflow - r0.n_overflow
            print("batch %d %s round=%s: worst rel %.3g, handed back %d (allowed %d)" % (which, ambigs, round_, rel, extra, allowed))
            assert rel <= REL_TOL
            assert np.array_equal(r.ns, ns) and np.array_equal(r.passed, ps.astype(bool))
            assert extra <= allowed
            if which == 0 and not round_:
                assert guarded_by_range == 0 and int(near_limit.sum()) == 0
                assert (r.ee != r0.ee).sum() > n // 2          # bit-equality everywhere would mean the exact body ran


def test_decisions_stay_exact_with_thresholds_on_reads_values(eng, oracle):
    q, lens = oracle.synth_fill(6000, 320, fixed_len=300, seed=8)
    ee0, _, _, _ = oracle.filter_batch(q, fixed_len=300, threads=8, ambigs="ignore")
    picks = [float(x) for x in np.unique(ee0[(ee0 > 0.5) & (ee0 < 60)])[::97][:12]]
    assert len(picks) >= 8
    for me in picks:
        on_threshold = int((ee0 == me).sum())
        assert on_threshold >= 1
        for kw in (dict(maxerrors=me, ambigs="ignore"), dict(maxerrors=me, ambigs="ignore", round_=True)):
            ee, ns, ps, _ = oracle.filter_batch(q, fixed_len=300, threads=8, **kw)
            r = eng.filter(q, fixed_len=300, odds=True, **kw)
            assert np.array_equal(r.passed, ps.astype(bool)), (me, kw)
            assert worst_rel(r.ee, ee) <= REL_TOL
            assert r.n_overflow >= on_threshold, (me, kw, r.n_overflow)
    for k in (10, 200, 999):
        u = float(ee0[k] / 300.0)
        if 0 < u <= 1:
            ee, ns, ps, _ = oracle.filter_batch(q, fixed_len=300, threads=8, uncert=u, ambigs="ignore")
            r = eng.filter(q, fixed_len=300, odds=True, uncert=u, ambigs="ignore")
            assert np.array_equal(r.passed, ps.astype(bool)), u


@pytest.mark.parametrize("name", G.NPZ_SETS)
def test_reference_vectors_within_tolerance(eng, name):
    s = G.load_set(name)
    alpha = float(s["alpha"])
    if alpha < 1e-5:
        with pytest.raises(ValueError, match="MPB_FLAG_ODDS needs alpha >= 1e-5"):
            eng.filter(s["q"], lens=s["lens"], alpha=alpha, ambigs="ignore", odds=True)
        return
    r = eng.filter(s["q"], lens=s["lens"], alpha=alpha, ambigs="ignore", odds=True)
    rel = worst_rel(r.ee, G.expected_value(s))
    print("%s: worst rel %.3g, n_overflow %d" % (name, rel, r.n_overflow))
    assert rel <= REL_TOL
    assert np.array_equal(r.ns, s["ns_ref"])
    if name == "long_reads":
        assert int((log2_p0(s["q"], s["lens"]) < -900).sum()) == 6 and np.isfinite(r.ee).all()


def test_reads_whose_ee_is_a_tiny_fraction(eng, oracle):
    """Short reads of random scores 1..254 (tests/test_odds_model.py has the same batch): ee down to 1e-9 and less, where only
    the unscaled numerator thr - p0 * lo keeps the relative tolerance."""
    rng = np.random.default_rng(5)
    q = rng.integers(1, 255, (20000, 16)).astype(np.uint8)
    for alpha in (1e-5, 0.001):
        ee, ns, ps, _ = oracle.filter_batch(q, fixed_len=12, threads=8, ambigs="ignore", alpha=alpha, maxerrors=3.0)
        r0 = eng.filter(q, fixed_len=12, ambigs="ignore", alpha=alpha, maxerrors=3.0)
        r = eng.filter(q, fixed_len=12, ambigs="ignore", alpha=alpha, maxerrors=3.0, odds=True)
        assert worst_rel(r.ee, ee) <= REL_TOL
        assert np.array_equal(r.passed, ps.astype(bool)) and np.array_equal(r.ns, ns)
        near_limit = int((np.abs(ee - 3.0) <= 1e-8 * np.maximum(1.0, np.abs(ee))).sum())
        print("alpha %g: handed back %d more than the exact mode's %d (allowed %d)" % (alpha, r.n_overflow - r0.n_overflow, r0.n_overflow, near_limit))
        assert r.n_overflow - r0.n_overflow <= near_limit


def test_flag_combinations_the_library_refuses(eng, oracle):
    q, _ = oracle.synth_fill(100, 320, fixed_len=300, seed=4)
    from moira_amd import _lib as L
    prm = eng.params(odds=True)
    prm.flags |= L.FLAG_FAST_FMA
    with pytest.raises(ValueError, match="MPB_FLAG_ODDS and MPB_FLAG_FAST_FMA"):
        eng.filter(q, fixed_len=300, params=prm)
    with pytest.raises(ValueError, match="MPB_FLAG_ODDS needs alpha >= 1e-5"):
        eng.filter(q, fixed_len=300, odds=True, alpha=1e-6)
    for kw in (dict(decision_only=True), dict(count_cells=True), dict(test_underpredict=True), dict(no_narrow=True)):
        ee, ns, ps, _ = oracle.filter_batch(q, fixed_len=300, threads=8)
        r = eng.filter(q, fixed_len=300, odds=True, **kw)
        assert np.array_equal(r.passed, ps.astype(bool)), kw
        fin = np.isfinite(r.ee)                                  # decision_only reports +inf for reads it settles
        assert worst_rel(r.ee[fin], ee[fin]) <= REL_TOL, kw


def test_edge_reads_the_range_guard(eng, oracle):
    """300 x Q2 (212 rows; P0 = 2^-431, inside the range) and 600 x Q1 (P0 = 0.206^600 = 2^-1368: under the guard, handed to
    the three-rounding pass), among ordinary reads: correct ee, no infinity or NaN leaks out."""
    q, lens = oracle.synth_fill(256, 608, min_len=50, max_len=600, seed=11)
    q[0, :] = 0; q[0, :300] = 2; lens[0] = 300
    q[1, :] = 0; q[1, :600] = 1; lens[1] = 600
    assert -450 < log2_p0(q[:1], lens[:1])[0] < -400 and log2_p0(q[1:2], lens[1:2])[0] < -1300
    for alpha in (0.005, 1e-5, 0.5):
        ee, ns, ps, rows = oracle.filter_batch(q, lens=lens, threads=8, alpha=alpha, uncert=1.0)
        r0 = eng.filter(q, lens=lens, alpha=alpha, uncert=1.0)
        r = eng.filter(q, lens=lens, alpha=alpha, uncert=1.0, odds=True)
        assert np.isfinite(r.ee).all() and np.isfinite(ee).all()
        assert worst_rel(r.ee, ee) <= REL_TOL
        assert np.array_equal(r.passed, ps.astype(bool)) and np.array_equal(r.ns, ns)
        assert r.ee[1] == ee[1]                                  # recomputed by the exact pass: bit for bit
        assert r.n_overflow >= r0.n_overflow + 1
        assert alpha != 0.005 or rows[0] >= 200


def test_device_resident_and_classified_entries(eng, oracle):
    n, stride, L = 50000, 320, 300
    d_q = eng.alloc(n * stride)
    eng.synth_fill(d_q, n, stride, fixed_len=L, seed=2, first_read=1000)
    host_q, _ = oracle.synth_fill(n, stride, fixed_len=L, seed=2, first_read=1000)
    ee, ns, ps, _ = oracle.filter_batch(host_q, fixed_len=L, threads=8)
    d_ee, d_ns, d_pass = eng.alloc(n * 8), eng.alloc(n * 4), eng.alloc(n)
    prm = eng.params(odds=True)
    c = eng.filter_device(d_q, n, stride, fixed_len=L, d_ee=d_ee, d_ns=d_ns, d_pass=d_pass, params=prm)
    got = d_ee.download(np.float64, n)
    assert worst_rel(got, ee) <= REL_TOL and (got != ee).sum() > n // 2
    assert np.array_equal(d_ns.download(np.int32, n), ns) and np.array_equal(d_pass.download(np.uint8, n), ps)
    assert (c.n_reads, c.n_pass) == (n, int(ps.sum())) and c.n_overflow < n // 100
    # classified at source: text -> decode + classify -> mpb_filter_device_classified, with the flag in both calls
    d_seq, d_qual, d_out = eng.alloc(n * stride), eng.alloc(n * stride), eng.alloc(n * stride)
    eng.encode_ascii_device(d_q, n, stride, d_seq, d_qual)
    d_ee.upload(np.full(n, -7.0)); d_pass.upload(np.full(n, 9, np.uint8))
    c2 = eng.filter_ascii_device(d_seq, d_qual, n, stride, d_out, fixed_len=L, d_ee=d_ee, d_ns=d_ns, d_pass=d_pass, params=prm)
    assert c2.n_pass == c.n_pass
    got2 = d_ee.download(np.float64, n)
    assert same(got2, got)
    assert np.array_equal(d_pass.download(np.uint8, n), ps)
    for b in (d_q, d_ee, d_ns, d_pass, d_seq, d_qual, d_out):
        b.free()


def test_private_table_and_small_batches_fall_back_to_the_exact_pass(eng, oracle):
    rng = np.random.default_rng(3)
    seqs = ["".join(rng.choice(list("ACGT"), 120)) for _ in range(6000)]
    quals = [[int(v) for v in rng.integers(2, 41, 120)] for _ in range(6000)]
    for k in range(0, 6000, 7):
        quals[k][5] = 300
        quals[k][77] = 5000
    q, lens, codes = eng.pack_coded(seqs, quals)
    assert (codes[1:255] != np.arange(1, 255)).sum() >= 2
    r0 = eng.filter(q, lens=lens, code_scores=codes)
    r = eng.filter(q, lens=lens, code_scores=codes, odds=True)
    assert same(r.ee, r0.ee) and np.array_equal(r.passed, r0.passed) and r.n_overflow == r0.n_overflow
    q, _ = oracle.synth_fill(3000, 320, fixed_len=300, seed=4)
    r0 = eng.filter(q, fixed_len=300, batched_only=False)
    r = eng.filter(q, fixed_len=300, batched_only=False, odds=True)
    assert same(r.ee, r0.ee) and np.array_equal(r.passed, r0.passed)
    assert (eng.filter(q, fixed_len=300, odds=True).ee != r0.ee).any()          # the batched path does run the mode


def test_the_flag_keeps_a_batch_out_of_the_narrow_pass(eng, oracle):
    n = 1 << 19
    q, _ = oracle.synth_fill(n, 320, fixed_len=300, seed=5, profile=1)
    d_q, d_ee, d_ns, d_pass = eng.alloc(n * 320).upload(q), eng.alloc(n * 8), eng.alloc(n * 4), eng.alloc(n)
    eng.filter_device(d_q, n, 320, fixed_len=300, d_ee=d_ee, d_ns=d_ns, d_pass=d_pass, params=eng.params())
    assert eng.last_path()["narrow_rows"] >= 2
    exact = d_ee.download(np.float64, n)
    eng.filter_device(d_q, n, 320, fixed_len=300, d_ee=d_ee, d_ns=d_ns, d_pass=d_pass, params=eng.params(odds=True))
    assert eng.last_path()["narrow_rows"] == 0
    assert worst_rel(d_ee.download(np.float64, n), exact) <= REL_TOL
    for b in (d_q, d_ee, d_ns, d_pass):
        b.free()
