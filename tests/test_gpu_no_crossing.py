"""The legitimate "CDF never crosses 1 - alpha" result (the reference's ReturnedNaNError, moira/moira.py:456,818) on the GPU.

Below alpha ~ 1e-15 the threshold 1 - alpha is a few ulp under 1 (exactly 1 below 1.1e-16), and whether a read's summed CDF ever
exceeds it is decided by the last bit of a sum over up to len + 1 rows: a dense, deterministic mix of reads with a result and
reads without one.  Every entry of the library must agree with the oracle on which is which -- never crossed in the main pass,
overflow list, final pass with NaN, pass = 2 and the host's re-run in the one-read-per-wave path, the hand-back of every narrow
form -- and bit for bit on the values.  Where 1 - alpha is exactly 1, Phi^-1 has no value; the host then hands the kernels
finite predictor constants that mean "every row", so every budget is all of a read's rows and only a read that never crosses
is re-run: mpb_filter_counts.n_overflow is then exactly the number of reads without a result."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import golden_io as G
from helpers.device_runs import Resident, classified_pair, same, seq_and_quals

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALPHAS = [1e-12, 1e-15, 1.2e-16, 1e-17, 1e-300]


@pytest.fixture(scope="module")
def eng():
    from moira_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def _random_batch():
    """4,000 reads of 0 .. 300 bases, every score drawn from Q1 .. Q41."""
    rng = np.random.default_rng(20161017)
    n = 4000
    lens = rng.integers(0, 301, n).astype(np.int32)
    q = rng.integers(1, 42, (n, 304)).astype(np.uint8)
    q[np.arange(304)[None, :] >= lens[:, None]] = 0
    return q, lens


def _fixed_batch():
    """3,000 reads of 300 bases, each around a quality level of its own (Q2 .. Q60), some with 'N' / 'n', a few of only 'N'."""
    rng = np.random.default_rng(20161018)
    n = 3000
    level = rng.integers(2, 61, n)
    q = np.clip(level[:, None] + rng.integers(-1, 2, (n, 320)), 1, 254).astype(np.uint8)
    q[::7, 5] = 0
    q[::11, 17] = 255
    q[::501, :] = 0
    q[:, 300:] = 0
    return q


def _long_batch():
    """32 reads of up to 4,096 bases at stride 4096: up to 4,097 rows (k_wide, four waves), good and bad ones."""
    rng = np.random.default_rng(20161019)
    spec = [(4096, 1, 3), (4096, 30, 41), (3000, 1, 4), (2500, 10, 25), (1500, 1, 3), (1025, 1, 2), (1024, 20, 41), (700, 1, 41)]
    q = np.zeros((32, 4096), np.uint8)
    lens = np.zeros(32, np.int32)
    for i in range(32):
        L, lo, hi = spec[i % 8]
        L = L if i < 8 else int(rng.integers(L // 2, L + 1))
        q[i, :L] = rng.integers(lo, hi, L)
        lens[i] = L
    q[3, 100] = 0
    q[5, 1000] = 255
    return q, lens


@pytest.fixture(scope="module")
def inputs():
    s = G.load_set("rand_mixed")
    q, lens = _random_batch()
    ql, ll = _long_batch()
    return {"random": (q, lens), "rand_mixed": (s["q"], s["lens"]), "long": (ql, ll)}


@pytest.fixture(scope="module")
def want(oracle, inputs):
    """{(input, alpha): (ee, ns, pass, rows)}, computed on first use and shared."""
    cache = {}

    def get(name, alpha, **kw):
        key = (name, alpha, tuple(sorted(kw.items())))
        if key not in cache:
            if name == "fixed":
                cache[key] = oracle.filter_batch(_fixed_batch(), fixed_len=300, alpha=alpha, threads=16, **kw)
            else:
                cache[key] = oracle.filter_batch(inputs[name][0], lens=inputs[name][1], alpha=alpha, threads=16, **kw)
        return cache[key]
    return get


def check(got, exp, label):
    ee, ns, ps = got[:3]
    nan = np.isnan(exp[0])
    assert np.array_equal(np.isnan(ee), nan), (label, int(np.isnan(ee).sum()), int(nan.sum()))
    assert same(ee, exp[0]), label
    assert np.array_equal(ns, exp[1]) and np.array_equal(np.asarray(ps).astype(bool), exp[2].astype(bool)), label
    assert not np.asarray(ps)[nan].any()


def test_the_inputs_hold_reads_of_both_kinds(want):
    """A condition on the inputs, checked on the oracle: at alpha 1e-15 at least a quarter of the random batch has no result
    and at least 5 % has one; the share grows as alpha shrinks and stays below 1 (reads without a scored base are 0)."""
    nan = np.isnan(want("random", 1e-15)[0])
    assert nan.mean() >= 0.25 and (~nan).mean() >= 0.05, nan.mean()
    assert not np.isnan(want("random", 1e-12)[0]).any()
    for name in ("random", "rand_mixed", "long"):
        shares = [np.isnan(want(name, a)[0]).mean() for a in ALPHAS[1:]]
        assert shares == sorted(shares) and shares[0] > 0.1 and shares[-1] < 1.0, (name, shares)
    assert int(want("long", 1e-17)[3].max()) == 4097               # every row of a 4,096-base read, and one more


@pytest.mark.parametrize("alpha", ALPHAS)
def test_sorted_pipeline_and_its_final_pass(eng, inputs, want, alpha):
    for name, (q, lens) in inputs.items():
        for under in (False, True):
            r = eng.filter(q, lens=lens, alpha=alpha, batched_only=True, no_narrow=True, test_underpredict=under)
            exp = want(name, alpha)
            check((r.ee, r.ns, r.passed), exp, (name, alpha, under))
            assert r.n_pass == int(exp[2].sum())
            # a read without a result was on the overflow list: it never crossed in the main pass, whatever its budget
            n_nan = int(np.isnan(exp[0]).sum())
            assert r.n_overflow >= n_nan
            if 1.0 - alpha == 1.0 and not under:
                # every budget, tile or wide, is all of the read's rows (scored + 1): nothing but a read that never crosses
                # can miss it, so the counter IS the number of reads without a result -- wide reads included ("long")
                assert r.n_overflow == n_nan, (name, alpha)


@pytest.mark.parametrize("alpha", ALPHAS)
def test_small_path_and_the_hosts_rerun(eng, inputs, want, alpha):
    """One read per wave: a read that never crosses gets pass = 2 there, and the host sends the batch down the pipeline."""
    for name in ("random", "rand_mixed", "long"):       # "long": pass = 2 also comes from the wide-read branch
        q, lens = inputs[name]
        assert len(lens) <= 4096
        for n in (len(lens), 200, 1):
            r = eng.filter(q[:n], lens=lens[:n], alpha=alpha)
            exp = [x[:n] for x in want(name, alpha)]
            check((r.ee, r.ns, r.passed), exp, (name, alpha, n))
            assert r.n_pass == int(exp[2].sum())


@pytest.mark.parametrize("alpha", ALPHAS)
def test_filter_device_without_counts_then_synchronise(eng, inputs, want, alpha):
    for name, (q, lens) in inputs.items():
        res = Resident(eng, q, lens)
        got = res.run(want_counts=False, alpha=alpha, no_narrow=True)
        res.free()
        check(got, want(name, alpha), (name, alpha))
        assert got[5]


@pytest.mark.parametrize("alpha", ALPHAS)
def test_classified_at_source_pair(eng, inputs, want, alpha):
    for name, (q, lens) in inputs.items():
        ee, ns, ps, c = classified_pair(eng, q, lens, alpha=alpha)
        check((ee, ns, ps), want(name, alpha), (name, alpha))
        assert c.n_pass == int(want(name, alpha)[2].sum())


@pytest.mark.parametrize("alpha", ALPHAS)
def test_every_forced_narrow_form_hands_them_back(eng, inputs, want, alpha):
    """The narrow pass finishes a read whose CDF crosses inside its R rows and hands every other one to the sorted pipeline:
    n_fallback = the reads that need more than R rows, or have no result at all, or hold an 'n' -- and, once 1 - alpha is
    exactly 1, the reads without a scored base (their row 0 is exactly 1, which does not exceed 1; the prepass settles them)."""
    fixed = _fixed_batch()
    q, lens = inputs["random"]
    for label, mat, ln, fl, name in (("fixed320", fixed, None, 300, "fixed"), ("fixed304", fixed[:, :304], None, 300, "fixed"),
                                     ("ragged304", q, lens, None, "random")):
        exp = want(name, alpha)
        ee0, rows = exp[0], exp[3]
        live = np.arange(mat.shape[1])[None, :] < (np.full(len(mat), fl) if ln is None else ln)[:, None]
        has_n = (live & (mat == 255)).any(1)
        back = np.isnan(ee0) | has_n
        res = Resident(eng, mat, ln)
        for R in (2, 3, 4):
            got = res.run(fixed_len=fl, alpha=alpha, narrow_rows=R)
            check(got, exp, (label, alpha, R))
            assert got[4]["narrow_rows"] == R and got[5]
            implied = back | (rows > R) | ((rows == 0) if 1.0 - alpha == 1.0 else False)
            assert got[4]["n_fallback"] == int(implied.sum()), (label, alpha, R)
            assert got[3].n_pass == int(exp[2].sum())
        res.free()


def _per_read_cases(inputs, k=200):
    q, lens = inputs["random"]
    return [seq_and_quals(q[i], int(lens[i])) + (a,) for i, a in zip(range(k), [1e-15, 1e-17] * (k // 2))]


def test_per_read_entry_resident_server(eng, oracle, inputs):
    """calculate_errors_PB read by read (k_serve): NaN where the oracle has NaN -- the wave reports pass = 2, the host runs the
    read alone through the pipeline."""
    n_nan = 0
    for seq, quals, alpha in _per_read_cases(inputs):
        ee, ns = eng.calculate_errors_PB(seq, quals, alpha)
        exp = oracle.ee_rowwise(seq, quals, alpha)
        assert same(np.float64(ee), np.float64(exp[0])) and ns == exp[1], (len(seq), alpha)
        n_nan += math.isnan(ee)
    assert 50 <= n_nan <= 190


def test_per_read_entry_launch_per_call(oracle, inputs):
    """The same 200 calls with MPB_SERVE=0 (read when a context first serves a per-read call, so: a process of its own)."""
    code = ("import sys, json; sys.path[:0] = [%r, %r]\n"
            "import golden_io as G\n"
            "from test_gpu_no_crossing import _per_read_cases, _random_batch\n"
            "from moira_amd.engine import Engine\n"
            "with Engine(0) as e: print(json.dumps([e.calculate_errors_PB(*r) for r in _per_read_cases({'random': _random_batch()})]))\n"
            % (ROOT, os.path.join(ROOT, "tests")))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=ROOT,
                       env=dict(os.environ, MPB_SERVE="0"))
    assert r.returncode == 0, r.stderr[-1500:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    exp = [oracle.ee_rowwise(*c)[:2] for c in _per_read_cases(inputs)]
    assert len(got) == 200
    for g, e in zip(got, exp):
        assert same(np.float64(g[0]), np.float64(e[0])) and g[1] == e[1]


@pytest.mark.parametrize("alpha", ALPHAS)
def test_decision_only_gives_infinity_where_its_bound_settles_and_nan_elsewhere(eng, inputs, want, alpha):
    """include/moira_pb.h, MPB_FLAG_DECISION_ONLY: the Chernoff test runs in the prepass, BEFORE any DP, so a read it settles is
    reported ee = +infinity, pass = 0 whether or not its CDF would ever have crossed; every read it does not settle is run, and
    one whose CDF never crosses is NaN, pass = 0.  Decisions are the full computation's either way.  The bound is restated here
    in double (mu = sum of p; settled when mu > 1 and floor(mu (1 - 1e-4) - clow sqrt(mu) - 0.02) > len x uncert, clow =
    1.0001 sqrt(2 ln(1 / (1 - alpha)))), and reads within 0.01 + 1e-5 mu of its edges -- the kernel sums mu in float -- are left out."""
    clow = math.sqrt(2 * math.log(1 / (1 - alpha))) * 1.0001
    seen_inf = seen_nan = False
    for name in ("random", "rand_mixed", "long"):
        q, lens = inputs[name]
        exp = want(name, alpha)
        r = eng.filter(q, lens=lens, alpha=alpha, decision_only=True, batched_only=True)
        assert np.array_equal(r.passed, exp[2].astype(bool)) and np.array_equal(r.ns, exp[1])
        inf = np.isposinf(r.ee)
        assert not r.passed[inf].any() and same(r.ee[~inf], exp[0][~inf])
        live = np.arange(q.shape[1])[None, :] < lens[:, None]
        p = np.where(live & (q != 0) & (q != 255), 10.0 ** (q / -10.0), 0.0)
        mu = p.sum(1)
        t = mu * (1 - 1e-4) - clow * np.sqrt(mu) - 0.02
        clear = (np.abs(t - np.rint(t)) > 0.01 + 1e-5 * mu) & (np.abs(mu - 1) > 0.01)
        settled = (mu > 1) & (np.floor(t) > lens * 0.01)
        assert np.array_equal(inf[clear], settled[clear]), (name, alpha)
        nan = np.isnan(exp[0])
        seen_inf |= bool((inf & nan).any())
        seen_nan |= bool((np.isnan(r.ee) & nan).any())
    if alpha <= 1e-15:                   # among the no-crossing reads: the long ones are settled, short good ones are not
        assert seen_inf and (seen_nan or alpha == 1e-15)


def test_reference_fixture_at_tiny_alpha(eng):
    """tests/golden/edge_alpha_tiny.npz: the reference's Python twin at alpha 1e-15 and 1e-17, NaN where its CDF never
    crosses, 0 for the reads without a scored base."""
    s = G.load_tiny_alpha()
    n = len(s["lens"])
    for ai, alpha in enumerate(float(a) for a in s["alphas"]):
        exp = s["ee_py"][ai]
        for kw in (dict(batched_only=True, no_narrow=True), dict(batched_only=True, test_underpredict=True), dict()):
            r = eng.filter(s["q"], lens=s["lens"], alpha=alpha, ambigs="ignore", **kw)
            assert same(r.ee, exp), (alpha, kw, int((np.isnan(r.ee) != np.isnan(exp)).sum()))
            assert np.array_equal(r.ns, s["ns_ref"]) and not r.passed[np.isnan(exp)].any()
        res = Resident(eng, s["q"], s["lens"])
        for R in (2, 4):
            got = res.run(alpha=alpha, ambigs="ignore", narrow_rows=R)
            assert same(got[0], exp) and got[4]["narrow_rows"] == R, (alpha, R)
        res.free()
        for i in range(0, n, 4):
            seq, quals = seq_and_quals(s["q"][i], int(s["lens"][i]))
            ee, ns = eng.calculate_errors_PB(seq, quals, alpha)
            assert same(np.float64(ee), exp[i]) and ns == s["ns_ref"][i], (alpha, i)


def test_opt_in_arithmetics_stay_refused_below_1e_5(eng, inputs):
    q, lens = inputs["random"]
    for kw in (dict(fast_fma=True), dict(odds=True)):
        with pytest.raises(ValueError, match="alpha >= 1e-5"):
            eng.filter(q[:64], lens=lens[:64], alpha=1e-15, **kw)
