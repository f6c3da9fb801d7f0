"""Directed inputs for k_wide, the kernel of every read that needs more than 1024 DP rows: the batches of
tests/helpers/wide_cells.py through every entry of the library, bit for bit against the oracle.  The ladder puts a crossing on
both sides of every wave boundary of all four instances (W = 2, 4, 8, 16 waves per workgroup) up to the last supported row, in
the main pass and -- with MPB_FLAG_TEST_UNDERPREDICT -- in the FINAL pass; reads at the instance edges, at the 64-base block
edges and at the full row stride, with random bytes behind every read's end; and a list batch of more than 2048 wide reads, so
that every workgroup of the grid takes a second trip of the list loop on reused LDS state, stepping over the other instance's
reads.  The LEDGER -- from the oracle's rows, the lengths and the budgets the library reports (0 = wide) -- says which cells
ran; an empty one fails by name."""
import numpy as np
import pytest

from helpers import front_end_model as FE
from helpers import wide_cells as WC
from helpers.device_runs import SENT_EE, SENT_NS, SENT_PS, Resident, classified_pair, same, seq_and_quals

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from moira_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def batches():
    return WC.generate()


def supported(exp):
    """The oracle's (ee, ns, pass, rows) as the library must give them: a read of more than 16384 rows has no result."""
    ee, ns, ps, rows = exp
    far = rows > WC.MAX_ROWS
    return np.where(far, np.nan, ee), ns, np.where(far, 0, ps).astype(np.uint8), rows


@pytest.fixture(scope="module")
def want(oracle, batches):
    """{batch name: (ee, ns, pass, rows)}: the oracle once per batch, one single-threaded call per worker."""
    return {b.name: supported(WC.oracle_results(oracle, b)) for b in batches}


def check(got, exp, label):
    ee, ns, ps = got[:3]
    bad = np.nonzero(~((ee == exp[0]) | (np.isnan(ee) & np.isnan(exp[0]))))[0]
    assert len(bad) == 0, (label, "%d reads differ; their rows J: %s" % (len(bad), sorted(int(j) for j in exp[3][bad])[:64]),
                           [(int(i), float(ee[i]), float(exp[0][i])) for i in bad[:4]])
    assert same(ee, exp[0]) and np.array_equal(ns, exp[1]), label
    assert np.array_equal(np.asarray(ps).astype(np.uint8), exp[2].astype(np.uint8)), label
    assert not (np.asarray(ee) == SENT_EE).any() and not (np.asarray(ns) == SENT_NS).any() and not (np.asarray(ps) == SENT_PS).any()


def timed_run(eng, res, **kw):
    """Resident.run with kernel timing on -> (its tuple, launches of k_wide)."""
    eng.timing(True)
    eng.timing_reset()
    try:
        out = res.run(no_narrow=True, **kw)
        return out, eng.kernel_times()["wide"][1]
    finally:
        eng.timing(False)


@pytest.fixture(scope="module")
def device_runs(eng, batches):
    """Every directed batch through mpb_filter_device, plain and with MPB_FLAG_TEST_UNDERPREDICT:
    {name: {under: (ee, ns, pass, counts, budgets, launches of k_wide)}}."""
    out = {}
    for b in batches:
        res = Resident(eng, b.q, b.lens)
        out[b.name] = {}
        for under in (False, True):
            (ee, ns, ps, c, path, intact), launches = timed_run(eng, res, alpha=b.alpha, test_underpredict=under)
            assert intact and path["narrow_rows"] == 0, (b.name, under)
            out[b.name][under] = (ee, ns, ps, c, eng.read_budgets(b.n), launches)
        res.free()
    return out


# ---- the directed batches through mpb_filter_device --------------------------------------------------------------------

@pytest.mark.parametrize("under", [False, True])
@pytest.mark.parametrize("name", WC.BATCH_NAMES)
def test_filter_device_is_the_oracle(batches, want, device_runs, name, under):
    b = [b for b in batches if b.name == name][0]
    exp = want[name]
    far = exp[3] > WC.MAX_ROWS
    assert far.sum() == (1 if b.stride == WC.STRIDES[-1] else 0)                                # the read beyond the range
    got = device_runs[name][under]
    check(got, exp, (name, under))
    assert np.array_equal(np.isnan(got[0]), far) and not got[2][far].any(), (name, under)      # NaN: that read alone
    assert (got[3].n_reads, got[3].n_pass) == (b.n, int(exp[2].sum())), (name, under)
    assert got[5] > 0, (name, under)                                                             # k_wide was launched


def test_budgets_are_zero_for_exactly_the_surely_wide_reads(batches, device_runs):
    """mpb_last_read_budgets: 0 for the reads the float64 model calls surely wide, the model's cap for its sure tile reads; no
    read of these batches is unsure, plain or halved."""
    for b in batches:
        for under in (False, True):
            m = WC.Rows(b.q, b.lens, b.alpha, underpredict=under)
            budgets = device_runs[b.name][under][4]
            assert (m.sure_wide | m.sure_tile).all(), (b.name, under)
            assert np.array_equal(budgets == 0, m.sure_wide), (b.name, under)
            assert np.array_equal(budgets[m.sure_tile], m.cap[m.sure_tile]), (b.name, under)


def test_n_overflow_counts_the_reads_whose_budget_missed(batches, want, device_runs):
    """Plain, only the read beyond the range misses (it never crosses inside sixteen waves).  Halved, the count lies inside
    front_end_model.overflow_bracket, and equals the number of provable misses where every read provably misses or holds."""
    total = 0
    for b in batches:
        rows = want[b.name][3]
        m = WC.Rows(b.q, b.lens, b.alpha)
        plain = int((m.sure_wide & (rows > WC.WAVE_ROWS * m.nw)).sum() + (m.sure_tile & (rows > m.cap)).sum())
        assert device_runs[b.name][False][3].n_overflow == plain == int((rows > WC.MAX_ROWS).sum()), b.name
        c = device_runs[b.name][True][3]
        lo, hi = FE.overflow_bracket(FE.Model(b.q, b.lens, b.alpha, underpredict=True), rows)
        assert lo <= c.n_overflow <= hi, (b.name, lo, c.n_overflow, hi)
        miss, holds = WC.misses_halved(b.q, b.lens, b.alpha, rows)
        assert (miss | holds).all(), b.name
        assert c.n_overflow == int(miss.sum()), (b.name, c.n_overflow, int(miss.sum()))
        total += c.n_overflow
    assert total >= 50


def test_no_cell_is_empty(batches, want, device_runs):
    """The ledger from the oracle's rows, the lengths and the budgets the library reported for both runs."""
    filled = set()
    for b in batches:
        ee, _, _, rows = want[b.name]
        filled |= WC.ledger(b, rows, nan=np.isnan(ee) & (rows <= WC.MAX_ROWS), budgets=device_runs[b.name][False][4],
                            budgets_under=device_runs[b.name][True][4])
    filled = WC.fold(filled)
    miss = WC.missing(WC.required_cells(), filled)
    assert not miss, "k_wide cells no read reached: %s" % miss
    count = {g: sum(1 for c in WC.required_cells() if WC.group_of(c) == g) for g in WC.GROUPS if g != "trips"}
    print("k_wide cells filled, per group: %s" % count)


# ---- the other entries ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("under", [False, True])
def test_host_entry_sorted_pipeline(eng, batches, want, device_runs, under):
    for b in batches:
        r = eng.filter(b.q, lens=b.lens, alpha=b.alpha, batched_only=True, no_narrow=True, test_underpredict=under)
        check((r.ee, r.ns, r.passed), want[b.name], (b.name, under))
        assert r.n_pass == int(want[b.name][2].sum()) and r.n_overflow == device_runs[b.name][under][3].n_overflow
        assert np.array_equal(eng.read_budgets(b.n), device_runs[b.name][under][4]), b.name


@pytest.mark.parametrize("under", [False, True])
def test_host_entry_one_read_per_wave_hands_the_batch_back(eng, batches, want, under):
    """Without MPB_FLAG_BATCHED_ONLY the one-read-per-wave kernel answers pass = 2 for a wide read and the host sends the batch
    down the pipeline (which classifies first: the launches of the classification pass show it)."""
    for b in batches:
        eng.timing(True)
        eng.timing_reset()
        try:
            r = eng.filter(b.q, lens=b.lens, alpha=b.alpha, test_underpredict=under)
            times = eng.kernel_times()
        finally:
            eng.timing(False)
        check((r.ee, r.ns, r.passed), want[b.name], (b.name, under))
        assert r.n_pass == int(want[b.name][2].sum())
        assert times["prepass"][1] > 0 and times["wide"][1] > 0, (b.name, under)


@pytest.mark.parametrize("under", [False, True])
def test_classified_at_source_pair(eng, batches, want, under):
    """mpb_decode_classify_device + mpb_filter_device_classified; that pair takes rows of up to 16384 bytes and refuses longer."""
    for b in batches:
        if b.stride > 16384:
            with pytest.raises(ValueError, match="16384"):
                classified_pair(eng, b.q, b.lens, alpha=b.alpha, test_underpredict=under)
            continue
        ee, ns, ps, c = classified_pair(eng, b.q, b.lens, alpha=b.alpha, test_underpredict=under)
        check((ee, ns, ps), want[b.name], (b.name, under))
        assert c.n_pass == int(want[b.name][2].sum())


def test_per_read_entry_on_one_read_per_instance(eng, batches, want):
    """bernoulli.calculate_errors_PB's twin on one ladder read of each instance (W = 2, 4, 8, 16) and on the last supported row."""
    done = []
    for J in (1025, 3073, 7169, 9217, WC.MAX_ROWS):
        L, k, tail = WC.LADDER[(WC.ALPHA, J)]
        b = [b for b in batches if b.alpha == WC.ALPHA and (want[b.name][3] == J).any()][0]
        i = int(np.nonzero(want[b.name][3] == J)[0][0])
        assert b.lens[i] == L + tail
        seq, quals = seq_and_quals(b.q[i], int(b.lens[i]))
        got = eng.calculate_errors_PB(seq, quals, b.alpha)
        assert got == (float(want[b.name][0][i]), int(want[b.name][1][i])), (J, got)
        done.append(WC.W_of(int(WC.nw_of(J))))
    assert done == [2, 4, 8, 16, 16]


# ---- modes and arithmetics, on the reads of at most 4096 rows --------------------------------------------------------------

@pytest.fixture(scope="module")
def small(batches, want):
    b = batches[0]
    sub, keep = WC.small_part(b, want[b.name][3])
    return sub, keep, tuple(x[keep] for x in want[b.name])


@pytest.mark.parametrize("kw", [dict(ambigs="ignore"), dict(ambigs="treat_as_errors", round_=True), dict(ambigs="disallow"),
                                dict(ambigs="ignore", round_=True), dict(ambigs="disallow", round_=True)],
                         ids=lambda kw: "-".join("%s" % v for v in kw.values()))
@pytest.mark.parametrize("under", [False, True])
def test_ambiguity_modes_and_round(eng, oracle, small, under, kw):
    sub = small[0]
    exp = oracle.filter_batch(sub.q, lens=sub.lens, alpha=sub.alpha, threads=8, **kw)
    assert exp[3].max() <= WC.SMALL_ROWS
    res = Resident(eng, sub.q, sub.lens)
    try:
        got = res.run(alpha=sub.alpha, no_narrow=True, test_underpredict=under, **kw)
    finally:
        res.free()
    check(got, exp, (kw, under))
    assert got[5] and got[3].n_pass == int(exp[2].sum())


@pytest.mark.parametrize("mode", [dict(odds=True), dict(fast_fma=True)], ids=["odds", "fast_fma"])
@pytest.mark.parametrize("under", [False, True])
def test_wide_reads_stay_exact_under_the_other_arithmetics(eng, small, under, mode):
    """k_wide has one arithmetic: with MPB_FLAG_ODDS or MPB_FLAG_FAST_FMA set, the wide reads of a batch keep their exact result
    (plain: the reads with budget 0; halved: also every read re-run by the FINAL pass, which is exact by construction)."""
    sub, _, exp = small
    res = Resident(eng, sub.q, sub.lens)
    try:
        ee, ns, ps, c, path, intact = res.run(alpha=sub.alpha, no_narrow=True, test_underpredict=under, **mode)
        budgets = eng.read_budgets(sub.n)
    finally:
        res.free()
    wide = budgets == 0
    if under:
        wide = wide | WC.misses_halved(sub.q, sub.lens, sub.alpha, exp[3], budgets)[0]
    assert intact and wide.sum() >= (10 if not under else sub.n - 2)
    check((ee[wide], ns[wide], ps[wide]), tuple(x[wide] for x in exp), (mode, under))
    assert np.array_equal(ns, exp[1])


# ---- the list batch: two trips of the list loop ------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def listed(oracle):
    b = WC.list_batch()
    exp = oracle.filter_batch(b.q, lens=b.lens, alpha=b.alpha, threads=8)
    return b, exp, WC.list_expect(b, exp[3])


@pytest.mark.parametrize("under", [False, True])
def test_trips_every_workgroup_takes_a_second_read(eng, listed, under):
    """More than 2 x 1024 reads in the list of the pass (plain: the main pass's wide list; halved: the overflow list, which
    the FINAL instances run): every read equals the oracle, no result slot keeps its sentinel, the guards are intact, and
    n_overflow is the count computed on the CPU.  The read of no bases is a tile read (a budget above 0, its CDF crosses in row 0):
    it reaches neither list."""
    b, exp, n_ovf = listed
    res = Resident(eng, b.q, b.lens)
    try:
        (ee, ns, ps, c, path, intact), launches = timed_run(eng, res, alpha=b.alpha, test_underpredict=under)
        budgets = eng.read_budgets(b.n)
    finally:
        res.free()
    check((ee, ns, ps), exp, ("list", under))
    assert intact and launches > 0
    assert c.n_overflow == n_ovf[under] and (c.n_reads, c.n_pass) == (b.n, int(exp[2].sum()))
    kw = dict(budgets=budgets) if not under else dict(budgets_under=budgets)
    assert ("wide", "final" if under else "main", "trips") in WC.ledger_trips(b, exp[3], **kw)
    empty = b.lens == 0
    assert empty.sum() == 1 and ee[empty][0] == 0.0 and budgets[empty][0] > 0


@pytest.mark.parametrize("under", [False, True])
def test_trips_host_entry_in_chunks(eng, listed, under):
    """The same batch through the host entry, whole and in three chunks (each chunk's lists are shorter than the grid)."""
    b, exp, n_ovf = listed
    r = eng.filter(b.q, lens=b.lens, alpha=b.alpha, batched_only=True, test_underpredict=under)
    check((r.ee, r.ns, r.passed), exp, ("list host", under))
    assert r.n_overflow == n_ovf[under]
    total = 0
    for lo in range(0, b.n, 800):
        sl = slice(lo, min(b.n, lo + 800))
        r = eng.filter(np.ascontiguousarray(b.q[sl]), lens=b.lens[sl], alpha=b.alpha, batched_only=True, test_underpredict=under)
        check((r.ee, r.ns, r.passed), tuple(x[sl] for x in exp), ("list chunk", lo, under))
        total += r.n_overflow
    assert total == n_ovf[under]
