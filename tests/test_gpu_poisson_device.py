"""The device tail of --error_calc poisson on the GPU (k_poisson_tail: mpb_poisson_finish_device, mpb_filter_poisson_device,
MPB_FLAG_POISSON_DEVICE_TAIL) against mpb_poisson_finish_host, the yardstick tests/test_poisson.py pins to the reference.
A read is EXACT when ee and pass equal the host tail's bit for bit (NaN at the same places), CLOSE when |ee - host| <= 1e-9 |host|
with an equal pass flag (where either side is 0, both are).  The input families are those of tests/test_poisson_device_model.py."""
import ctypes as C

import numpy as np
import pytest

import golden_io as G
from helpers import poisson_tail_model as P
from moira_amd import _lib as L

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from moira_amd.engine import Engine
    with Engine(0) as e:
        yield e


class Tail:
    """lambda / ns / len resident in HBM; one mpb_poisson_finish_device call per run."""

    def __init__(self, eng, lam, ns, lens=None):
        self.eng, self.n = eng, len(lam)
        n = max(1, self.n)
        self.ns = np.ascontiguousarray(ns, np.int32)
        self.lam = np.ascontiguousarray(lam, np.float64)
        self.d_lam, self.d_ns = eng.alloc(n * 8), eng.alloc(n * 4).upload(self.ns)
        self.d_len = eng.alloc(n * 4).upload(np.ascontiguousarray(lens, np.int32)) if lens is not None else None
        self.d_ee, self.d_pass = eng.alloc(n * 8), eng.alloc(n)

    def run(self, fixed_len=0, alias=False, **kw):
        """-> (ee, pass, counts, launches of k_poisson_tail)"""
        eng, n = self.eng, self.n
        self.d_lam.upload(self.lam)
        self.d_ee.upload(np.full(n, -7.0))
        self.d_pass.upload(np.full(n, 9, np.uint8))
        d_ee = self.d_lam if alias else self.d_ee
        eng.timing(True)
        eng.timing_reset()
        c = eng.poisson_finish_device(self.d_lam, self.d_ns, n, d_len=self.d_len if not fixed_len else None, fixed_len=fixed_len,
                                      d_ee=d_ee, d_pass=self.d_pass, params=eng.params(**kw))
        launches = eng.kernel_times()["poisson_tail"][1]
        eng.timing(False)
        assert np.array_equal(self.d_ns.download(np.int32, n), self.ns)                    # d_ns is untouched
        if not alias:
            assert np.array_equal(self.d_lam.download(np.float64, n), self.lam, equal_nan=True)
        return d_ee.download(np.float64, n), self.d_pass.download(np.uint8, n), c, launches

    def free(self):
        for b in (self.d_lam, self.d_ns, self.d_len, self.d_ee, self.d_pass):
            if b is not None:
                b.free()


@pytest.mark.parametrize("alpha", P.ALPHAS)
def test_lambda_grid_through_finish_device(eng, alpha):
    g = P.lambda_grid(alpha)
    n, lam = P.GRID_N, g["lam"]
    with np.errstate(invalid="ignore"):
        out_of_range = ~((lam >= 0) & (lam <= P.LAMBDA_MAX))
    t = Tail(eng, lam, g["ns"], g["lens"])
    fixed = np.full(n, 300, np.int32)
    try:
        for kw in P.settings((alpha,)):
            # ragged lengths into arrays of their own; fixed length 300 with d_ee aliasing d_lambda
            for lens, fixed_len, alias in ((g["lens"], 0, False), (fixed, 300, True)):
                hee, hps = P.host_tail(lam, g["ns"], lens, **kw)
                ee, ps, c, launches = t.run(fixed_len=fixed_len, alias=alias, **kw)
                assert launches == 1, kw                                                   # the mode ran
                ok = P.close(ee, ps, hee, hps)
                assert ok.all(), (kw, fixed_len, np.flatnonzero(~ok)[:5], lam[~ok][:5], ee[~ok][:5], hee[~ok][:5])
                assert P.exact(ee, ps, hee, hps)[out_of_range].all(), kw
                assert set(np.unique(ps)) <= {0, 1}
                assert c.n_reads == n and c.n_pass == int(ps.sum()) and c.n_fail == n - c.n_pass
                assert c.n_overflow >= g["n_range"], kw
                assert c.n_overflow - g["n_range"] - g["n_planted"] <= P.CAP_SHARE * n, (kw, c.n_overflow)
    finally:
        t.free()


def test_decisions_on_the_limit(eng):
    f = P.limit_family()
    lam, ns, lens = f["lam"], f["ns"], f["lens"]
    t = Tail(eng, lam, ns)
    try:
        hee, _ = P.host_tail(lam, ns, lens, alpha=0.005)
        picks = [k for k in range(len(hee)) if hee[k] > 0.5][:6]
        assert len(picks) == 6
        for k in picks:
            kw = dict(alpha=0.005, maxerrors=float(hee[k]))                                # the limit IS read k's own ee
            base = t.run(fixed_len=300, alpha=0.005, maxerrors=float(hee[k]) * 1.5)[2].n_overflow
            want_ee, want_ps = P.host_tail(lam, ns, lens, **kw)
            ee, ps, c, _ = t.run(fixed_len=300, **kw)
            assert P.close(ee, ps, want_ee, want_ps).all()
            assert ee[k] == want_ee[k] and ps[k] == want_ps[k] == 1
            assert c.n_overflow >= base + 1 and c.n_overflow >= int(P.model(lam, ns, lens, **kw)["c"].sum()) >= 1
    finally:
        t.free()
    lam = np.concatenate([P.integer_lambdas(), f["lam"][:994]])                           # ee within 1e-10 of 1, 2, .. 6
    t = Tail(eng, lam, ns)
    try:
        for ambigs in P.AMBIGS:
            kw = dict(alpha=0.005, round_=True, ambigs=ambigs)
            want_ee, want_ps = P.host_tail(lam, ns, lens, **kw)
            ee, ps, c, _ = t.run(fixed_len=300, **kw)
            assert P.close(ee, ps, want_ee, want_ps).all()
            assert P.exact(ee, ps, want_ee, want_ps)[:6].all() and c.n_overflow >= 6
    finally:
        t.free()


def _filter_device(eng, q, lens, fixed_len, with_lambda=True, **kw):
    n, stride = q.shape
    m = max(1, n)
    d_q = eng.alloc(max(16, q.nbytes)).upload(np.ascontiguousarray(q))
    d_len = eng.alloc(m * 4).upload(np.ascontiguousarray(lens, np.int32)) if lens is not None else None
    d_ee, d_ns, d_pass, d_lam = eng.alloc(m * 8), eng.alloc(m * 4), eng.alloc(m), eng.alloc(m * 8) if with_lambda else None
    try:
        c = eng.filter_poisson_device(d_q, n, stride, d_len=d_len, fixed_len=fixed_len, d_ee=d_ee, d_ns=d_ns, d_pass=d_pass,
                                      d_lambda=d_lam, params=eng.params(**kw))
        lam = d_lam.download(np.float64, n) if with_lambda else None
        if with_lambda:
            d_l2, d_n2 = eng.alloc(m * 8), eng.alloc(m * 4)
            L.check(eng.lib.mpb_poisson_lambda_device(eng.ctx, d_q.ptr, n, stride, d_len.ptr if d_len is not None else None, fixed_len,
                                                      d_l2.ptr, d_n2.ptr))
            assert np.array_equal(lam, d_l2.download(np.float64, n)) and np.array_equal(d_ns.download(np.int32, n), d_n2.download(np.int32, n))
            d_l2.free(); d_n2.free()
        return d_ee.download(np.float64, n), d_ns.download(np.int32, n), d_pass.download(np.uint8, n), c, lam
    finally:
        for b in (d_q, d_len, d_ee, d_ns, d_pass, d_lam):
            if b is not None:
                b.free()


@pytest.mark.parametrize("stride", P.MATRIX_STRIDES)
def test_matrix_to_result_through_filter_poisson_device(eng, stride):
    q, lens, full = P.matrix_family(stride)
    n = len(lens)
    for mat, ll, fixed_len in ((q, lens, 0), (full, None, stride)):
        for with_lambda, kw in ((True, dict(alpha=0.005)), (False, dict(alpha=1e-5, ambigs="ignore")), (True, dict(alpha=0.05, round_=True))):
            want = eng.filter_poisson(mat, lens=ll, fixed_len=None if ll is not None else fixed_len, **kw)
            ee, ns, ps, c, _ = _filter_device(eng, mat, ll, fixed_len, with_lambda=with_lambda, **kw)
            assert P.close(ee, ps, want.ee, want.passed).all(), (stride, kw)
            assert np.array_equal(ns, want.ns) and c.n_pass == want.n_pass == int(ps.sum()) and c.n_reads == n
            assert set(np.unique(ps)) <= {0, 1} and 0 <= c.n_overflow < n
    bad = q.copy()
    bad[5, 0] = 255
    l2 = lens.copy()
    l2[5] = max(1, l2[5])
    with pytest.raises(ValueError, match="255"):
        _filter_device(eng, bad, l2, 0, alpha=0.005)
    with pytest.raises(ValueError, match="alpha >= 1e-5"):
        _filter_device(eng, q, lens, 0, alpha=1e-6)
    # n = 0 and n = 1
    assert _filter_device(eng, q[:0], lens[:0], 0, with_lambda=False)[3].n_reads == 0
    one = eng.filter_poisson(full[7:8], fixed_len=stride)
    ee, ns, ps, c, _ = _filter_device(eng, full[7:8], None, stride)
    assert P.close(ee, ps, one.ee, one.passed).all() and ns[0] == one.ns[0] and c.n_reads == 1 and c.n_pass == int(ps[0])


def test_everything_handed_back(eng):
    for q, fixed_len in P.handed_back_family():
        n = len(q)
        want = eng.filter_poisson(q, fixed_len=fixed_len)
        ee, ns, ps, c, lam = _filter_device(eng, q, None, fixed_len)
        assert P.exact(ee, ps, want.ee, want.passed).all() and np.array_equal(ns, want.ns)
        assert c.n_overflow == n and c.n_pass == int(ps.sum()) == want.n_pass
        assert (lam > P.LAMBDA_MAX).all()
    assert np.isnan(ee).all() and np.isfinite(eng.filter_poisson(P.handed_back_family()[0][0], fixed_len=1024).ee).all()


def test_everything_handed_back_beyond_the_record_block(eng):
    """More handed-back reads than the kernel's record block holds (65536): the arrays travel whole, the results are the host's."""
    n = 70_001
    lam = np.random.default_rng(3).uniform(65, 150, n)
    lam[::1000] = 2.0                                                                      # a few reads the device keeps
    ns, lens = np.zeros(n, np.int32), np.full(n, 300, np.int32)
    t = Tail(eng, lam, ns)
    try:
        want_ee, want_ps = P.host_tail(lam, ns, lens, alpha=0.005)
        ee, ps, c, _ = t.run(fixed_len=300, alpha=0.005)
        assert P.close(ee, ps, want_ee, want_ps).all() and P.exact(ee, ps, want_ee, want_ps)[lam > 64].all()
        assert c.n_overflow == int((lam > 64).sum()) > 65536 and c.n_pass == int(ps.sum())
    finally:
        t.free()


def test_the_references_own_set(eng):
    """tests/golden/poisson.npz: moira.py's calculate_errors_poisson on 2,300 reads x its alphas."""
    z = G.load_set("poisson")
    seen = refused = 0
    for t in ("a", "b"):
        q, lens = z["q_" + t], z["lens_" + t]
        for ai, alpha in enumerate(z["alphas"]):
            if alpha < 1e-5:
                with pytest.raises(ValueError, match="alpha >= 1e-5"):
                    _filter_device(eng, q, lens, 0, alpha=float(alpha), ambigs="ignore")
                refused += 1
                continue
            ee, ns, ps, c, _ = _filter_device(eng, q, lens, 0, alpha=float(alpha), ambigs="ignore")
            o = z["ovf_" + t][ai].astype(bool)
            ref = z["ee_" + t][ai]
            assert np.array_equal(ns, z["ns_" + t])
            assert np.isnan(ee[o]).all() and not np.isnan(ee[~o]).any()
            assert (P.rel_err(ee[~o], ref[~o]) <= P.CONTRACT).all()
            assert c.n_overflow >= int(o.sum())
            seen += 1
    assert seen >= 2
    if not refused:                                 # no alpha below the floor in the file: the refusal is asked for directly
        with pytest.raises(ValueError, match="alpha >= 1e-5"):
            _filter_device(eng, z["q_a"], z["lens_a"], 0, alpha=1e-6, ambigs="ignore")


def test_host_pipeline_with_the_flag(eng, oracle):
    n = 300_017
    q, lens = oracle.synth_fill(n, 608, min_len=50, max_len=600, seed=5)
    kw = dict(alpha=0.005, ambigs="treat_as_errors")
    before = eng.filter_poisson(q, lens=lens, **kw)
    eng.timing(True)
    eng.timing_reset()
    r = eng.filter_poisson(q, lens=lens, poisson_device_tail=True, **kw)
    times = eng.kernel_times()
    eng.timing(False)
    assert times["poisson_tail"][1] == times["lambda"][1] == 4                            # four chunks, the tail behind each k_lambda
    ok = P.close(r.ee, r.passed, before.ee, before.passed)
    assert ok.all(), (np.flatnonzero(~ok)[:5], r.ee[~ok][:5], before.ee[~ok][:5])
    assert np.array_equal(r.ns, before.ns) and r.n_pass == before.n_pass == int(r.passed.sum())
    lam, _ = P.lambda_of(q, lens)
    beyond = int((lam > P.LAMBDA_MAX).sum())
    assert beyond <= r.n_overflow <= beyond + P.CAP_SHARE * n
    assert r.n_overflow >= int(np.isnan(before.ee).sum())                                  # every NaN came from the host tail
    assert (r.ee != before.ee)[~np.isnan(before.ee)].any()                                 # (the device arithmetic did run)
    bad = q.copy()
    bad[n - 5, 3] = 255                                                                    # a lower-case n in the LAST chunk
    with pytest.raises(ValueError, match="255"):
        eng.filter_poisson(bad, lens=lens, poisson_device_tail=True, **kw)
    with pytest.raises(ValueError, match="alpha >= 1e-5"):
        eng.filter_poisson(q[:100], lens=lens[:100], poisson_device_tail=True, alpha=1e-6)
    after = eng.filter_poisson(q, lens=lens, **kw)                                         # without the flag: what it was before
    assert np.array_equal(after.ee, before.ee, equal_nan=True) and np.array_equal(after.passed, before.passed)
    assert np.array_equal(after.ns, before.ns) and after.n_pass == before.n_pass and after.n_overflow == 0
