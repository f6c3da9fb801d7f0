"""The directed class-body inputs under MPB_FLAG_FAST_FMA and MPB_FLAG_ODDS.  mpb_dp_tiles.inc is compiled once per arithmetic,
so each of the 32 tile classes has a body of its own per mode -- its own hand-over of row j - 1 across a lane boundary, its own
end of a read -- and tests/test_gpu_class_edges.py reaches the exact ones only.  Here the batches of
tests/helpers/class_cells.py generate(mode=...) go through the library with the mode set, read by read and bit for bit against
the mode's CPU model (oracle/pb_oracle.c, pbo_filter_batch_model), or against the exact oracle where the mode's rules hand the
read to the three-rounding pass (tests/helpers/mode_expect.py, exact form).  The LEDGER is built from the budgets the library
reports and the model's rows; an empty required cell fails the test by name.  Then the two places where a mode's end of a read
decides: ODDS' range guard p0 >= 2^-900 at its boundary, and the 1e-9 band around a read's limit.  No tolerance anywhere."""
import numpy as np
import pytest

from helpers import class_cells as CC
from helpers import mode_expect as X
from helpers.device_runs import Resident
from helpers.opt_in_inputs import MODES, mode_kw

pytestmark = pytest.mark.gpu

THREADS = 16


@pytest.fixture(scope="module")
def eng():
    from moira_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def cpu_sides(oracle, b, mode, **kw):
    """(exact (ee, ns, pass), model) of one batch."""
    return (oracle.filter_batch(b.q, lens=b.lens, alpha=b.alpha, threads=THREADS, **kw)[:3],
            oracle.filter_batch_model(b.q, mode, lens=b.lens, alpha=b.alpha, threads=THREADS, **kw))


@pytest.fixture(scope="module")
def cpu(oracle):
    """mode -> [(batch, exact, model)], computed once per mode."""
    memo = {}

    def get(mode):
        if mode not in memo:
            memo[mode] = [(b,) + cpu_sides(oracle, b, mode) for b in CC.generate(oracle, mode=mode)]
        return memo[mode]
    return get


def device_run(eng, b, mode, **kw):
    """One batch through mpb_filter_device (sorted pipeline) -> ((ee, ns, pass), counts, budgets); guards intact."""
    res = Resident(eng, b.q, b.lens)
    try:
        ee, ns, ps, c, path, intact = res.run(fixed_len=b.fixed_len, alpha=b.alpha, no_narrow=True, **mode_kw(mode), **kw)
    finally:
        res.free()
    assert intact and path["narrow_rows"] == 0, b.name
    return (ee, ns, ps), c, eng.read_budgets(b.n)


@pytest.fixture(scope="module")
def main_runs(eng, cpu):
    """mode -> {batch name: ((ee, ns, pass), counts, budgets)} of the main pass, run once per mode."""
    memo = {}

    def get(mode):
        if mode not in memo:
            memo[mode] = {b.name: device_run(eng, b, mode) for b, _, _ in cpu(mode)}
        return memo[mode]
    return get


def required(oracle, mode):
    return CC.main_cells() if mode == "fma" else CC.odds_cells(oracle)


def joined(parts):
    return tuple(np.concatenate([p[k] for p in parts]) for k in range(len(parts[0])))


# ---- a. main pass ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
def test_main_pass_is_the_model_and_no_cell_is_empty(oracle, cpu, main_runs, mode):
    """Every read equals the model, or the exact oracle where the rule says so (n_overflow counts exactly those of the tile
    classes); from the real budgets, every required (class, crossing row) cell has a read that the mode's own body finished."""
    import pb_oracle
    filled = set()
    gots, exacts, models, left = [], [], [], []
    for b, exact, m in cpu(mode):
        got, c, budgets = main_runs(mode)[b.name]
        X.check_exact_form(got, exact, m, budgets, c.n_overflow)
        assert np.isin(budgets, np.r_[0, CC.CAPS]).all() and c.n_reads == b.n, b.name
        filled |= CC.ledger_mode(m, budgets)
        gots.append(got)
        exacts.append(exact)
        models.append(m)
        left.append(~X.expect(exact, m, budgets)["must_exact"])
    miss = CC.missing(required(oracle, mode), filled)
    assert not miss, "[%s] main cells no read reached (class, crossing row): %s" % (mode, miss)
    if mode == "fma":
        assert len(required(oracle, mode)) == 170
    else:
        assert all(c[1] == 1024 for c in CC.odds_unreachable(oracle))
    model = pb_oracle.ModelResult(**{k: np.concatenate([m.__dict__[k] for m in models]) for k in models[0].__dict__})
    gpu, cpu_share = X.check_mode_ran(joined(gots), joined(exacts), model, among=np.concatenate(left))
    print("[%s] %d batches, %d reads, %d cells filled of %d required; model != exact %.1f %% (GPU %.1f %%)" % (
        mode, len(gots), len(model.ee), len(set(required(oracle, mode)) & filled), len(required(oracle, mode)),
        100 * cpu_share, 100 * gpu))


# ---- b. overflow batches -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
def test_underpredicted_batches_follow_the_rule(eng, oracle, cpu, mode):
    """MPB_FLAG_TEST_UNDERPREDICT with a mode set: a read whose halved budget misses under the MODEL's rows goes to the overflow
    pass, which always runs the three-rounding arithmetic (no mode cell to fill there); the rest equal the model.  The exact
    overflow batches the modes accept (alpha >= 1e-5) and the mode's own stride-960 batches."""
    todo = [(b,) + cpu_sides(oracle, b, mode) for b in CC.generate(oracle) if b.kind == "ovf" and b.alpha >= min(CC.MODE_ALPHAS)]
    assert len(todo) >= 30
    todo += [t for t in cpu(mode) if t[0].stride == 960]
    misses = kept = 0
    for b, exact, m in todo:
        got, c, budgets = device_run(eng, b, mode, test_underpredict=True)
        _, miss, _ = X.check_exact_form(got, exact, m, budgets, c.n_overflow)
        misses += miss
        kept += int((~X.expect(exact, m, budgets)["must_exact"]).sum())
    print("[%s] %d batches under test_underpredict: %d budget misses, %d reads left to the mode" % (mode, len(todo), misses, kept))
    assert misses > 500, misses                   # about 1000 reads in all, nearly every one made to miss


# ---- c. host entry -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
def test_host_entry_is_the_device_run(eng, cpu, main_runs, mode):
    for b, _, _ in cpu(mode):
        got, c, budgets = main_runs(mode)[b.name]
        r = eng.filter(b.q, alpha=b.alpha, batched_only=True, no_narrow=True, **mode_kw(mode), **b.len_kw())
        assert X.matches(r.ee, r.ns, r.passed, got[0], got[1], got[2].astype(bool)).all(), b.name
        assert (r.n_overflow, r.n_pass) == (c.n_overflow, c.n_pass), b.name
        assert np.array_equal(eng.read_budgets(b.n), budgets), b.name


# ---- d. FAST_FMA on the one-read-per-wave bodies -----------------------------------------------------------------------------

def test_fast_fma_thin_bodies(eng, cpu, main_runs):
    """k_small<true>: the reads the mode keeps and whose budget holds, as a batch of their own without MPB_FLAG_BATCHED_ONLY.
    The one-read-per-wave kernel finishes it alone (no classification pass), every read equals the model, and the thin ledger
    from the real budgets fills all 28 cells.  (ODDS has no one-read form: the exact kernel runs, tested elsewhere.)"""
    filled = set()
    for b, exact, m in cpu("fma"):
        budgets = main_runs("fma")[b.name][2]
        keep = np.flatnonzero(~m.hand & (budgets > 0) & (m.rows >= 1) & (m.rows <= budgets))
        if b.stride > 2048 or len(keep) == 0:
            continue
        assert len(keep) <= 4096
        eng.timing(True)
        eng.timing_reset()
        try:
            r = eng.filter(np.ascontiguousarray(b.q[keep]), lens=b.lens[keep], alpha=b.alpha, fast_fma=True, batched_only=False)
            prepass = eng.kernel_times()["prepass"][1]
        finally:
            eng.timing(False)
        ok = X.matches(r.ee, r.ns, r.passed, m.ee[keep], exact[1][keep], m.passed[keep])
        assert ok.all(), (b.name, keep[~ok][:5].tolist())
        assert prepass == 0 and r.n_overflow == 0, (b.name, prepass)
        sub = type(m)(**{k: v[keep] for k, v in m.__dict__.items()})
        filled |= CC.ledger_thin_mode(sub, budgets[keep])
    miss = CC.missing(CC.thin_cells(), filled)
    assert not miss and len(CC.thin_cells()) == 28, "thin cells no read reached (body, crossing row): %s" % miss


# ---- e. ODDS' range guard at its boundary ------------------------------------------------------------------------------------

@pytest.mark.parametrize("cap", sorted(CC.GUARD_CORES))
def test_odds_range_guard_at_its_boundary(eng, oracle, cap):
    """Reads of one class whose p0 steps across 2^-900 one Q40 base (1.4e-4 bit) at a time, all within 0.05 bit of it: above,
    the ODDS body keeps the read (the model's bits); below, it reports the read as never crossed and the exact pass runs it
    (the exact oracle's bits, counted in n_overflow).  Nothing overflows on either side."""
    q, lens, _ = CC.range_guard_ladder(oracle, cap)
    b = CC.Batch("guard%d" % cap, "main", 0.005, q, lens)
    exact, m = cpu_sides(oracle, b, "odds")
    off = np.log2(m.p0) - CC.P0_MIN_LOG2
    assert (np.abs(off) <= CC.GUARD_BAND).all() and np.array_equal(m.hand, off < 0) and m.hand.any() and not m.hand.all()
    got, c, budgets = device_run(eng, b, "odds")
    assert (budgets == cap).all() and (m.rows <= budgets).all()
    X.check_exact_form(got, exact, m, budgets, c.n_overflow)
    assert np.isfinite(got[0]).all() and np.isfinite(m.ee).all()
    assert X.matches(*got, m.ee, exact[1], m.passed)[~m.hand].all()
    assert X.matches(*got, exact[0], exact[1], exact[2].astype(bool))[m.hand].all()
    assert c.n_overflow == int(m.hand.sum())
    assert X.differs(exact, m)[~m.hand].any()                   # above the boundary the model is not the exact oracle


# ---- f. the 1e-9 hand-over band ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
def test_the_1e_9_band_around_the_limit(eng, oracle, mode):
    """A class-160 batch with maxerrors set beside a read's own model ee: within 1e-9 relative the mode does not trust its ee
    and hands the read to the exact pass, at twice that distance it keeps it -- on the CPU model, and on the GPU by the
    exact-form rule, with --round as well."""
    q, lens = CC.band_batch()
    b = CC.Batch("band", "main", 0.005, q, lens)
    m0 = oracle.filter_batch_model(q, mode, lens=lens, threads=THREADS, ambigs="ignore")
    picks = CC.band_picks(m0)
    assert len(picks) == 3
    handed = 0
    for i in picks:
        e = float(m0.ee_model[i])
        for f, inside in CC.BAND_FACTORS:
            for me in (e * (1 - f), e * (1 + f)):
                for round_ in (False, True):
                    kw = dict(ambigs="ignore", maxerrors=me, round_=round_)
                    exact, m = cpu_sides(oracle, b, mode, **kw)
                    if not round_:
                        assert bool(m.hand[i]) == inside, (i, f, me)
                    got, c, budgets = device_run(eng, b, mode, **kw)
                    assert budgets[i] == 160 and m.rows[i] <= 160
                    X.check_exact_form(got, exact, m, budgets, c.n_overflow)
                    handed += int(m.hand[i])
    assert handed >= 12
