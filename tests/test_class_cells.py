"""The directed-input generator of tests/helpers/class_cells.py, on the CPU: its class table is the header's, it fills every
required cell under the predictor model and the oracle's rows, it is deterministic and its batches stay small.  (What the GPU
files assert never comes from the model: test_gpu_class_edges.py builds its ledger from the budgets the library reports.)"""
import os

import numpy as np
import pytest

from helpers import class_cells as CC
from helpers import mode_expect as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_READS = 20_000           # all directed batches together: the GPU files run every one of them through several entries
MAX_MODE_READS = 10_000      # the batches of both modes together


@pytest.fixture(scope="module")
def batches(oracle):
    return CC.generate(oracle)


def test_class_tables_are_the_headers():
    text = open(os.path.join(ROOT, "moira_amd", "csrc", "mpb_internal.h")).read()
    got = CC.parse_header_classes(text)
    assert got["MPB_CLASSES"] == list(CC.TILE_CLASSES) and len(CC.TILE_CLASSES) == 32
    assert got["MPB_THIN_CLASSES"] == list(CC.THIN_CLASSES) and len(CC.THIN_CLASSES) == 10
    assert all(g * r == cap and r <= 16 and 64 % g == 0 for cap, g, r in CC.TILE_CLASSES + CC.THIN_CLASSES)
    assert list(CC.CAPS) == sorted(set(int(c) for c in CC.CAPS)) and CC.CAPS[-1] == CC.TILE_MAX_ROWS
    assert [c[0] for c in CC.THIN_CLASSES] == [2 << k for k in range(10)]
    # every tile class lies inside one thin body's rows (prev, cap]: the tile budget names the thin body
    for cap, _, _ in CC.TILE_CLASSES:
        lo, hi = CC.prev_cap(cap) + 1, cap
        assert len({int(CC.thin_cap_of_budget(CC.cap_of_rows(r))) for r in (lo, hi)}) == 1
        want = 2 if hi <= 2 else 1 << (hi - 1).bit_length()
        assert int(CC.thin_cap_of_budget(cap)) == want == (2 if lo <= 2 else 1 << (lo - 1).bit_length())
    assert list(CC.cap_of_rows(np.array([1, 2, 3, 17, 1024, 1025]))) == [2, 2, 3, 20, 1024, 0]


def test_required_cell_counts():
    main = CC.main_cells()
    assert len(main) == len(set(main)) == 170
    assert ("main", 1024, 911) in main and ("main", 1024, 912) in main           # the lane boundary at g = 57
    assert ("main", 1024, 991) in main and ("main", 1024, 992) in main
    assert len(CC.overflow_cells_all()) == 108 and len(CC.thin_cells()) == 28 and len(CC.narrow_cells()) == 48


def test_unreachable_overflow_cells_are_out_of_every_inputs_reach(oracle):
    """A batch that selects class `cap` for its overflow pass holds reads of at most cap - 1 bases; even all of them Q1, at the
    smallest alpha at which such a read still has a result, need fewer rows than the first row of the last lane of the classes
    with G >= 32.  Only those three cells are dropped, each by that bound; the classes with G = 16 reach theirs below alpha
    1e-6, and get a batch at 1e-12 for it."""
    bad = CC.overflow_unreachable(oracle)
    assert bad == [("ovf", cap, (G - 1) * R) for cap, G, R in CC.TILE_CLASSES if G >= 32]
    for _, cap, js in bad:
        assert CC.overflow_max_rows(oracle, cap) < js + 1
        for alpha in (1e-13, 1e-14, 3e-15):                # nothing between the ladder's steps reaches it either
            assert CC.overflow_max_rows(oracle, cap, (alpha,)) < js + 1
    assert len(CC.overflow_cells(oracle)) == 105
    deep = [cap for cap, G, R in CC.TILE_CLASSES if G > 1 and CC.OVF_DEEP_ALPHA in CC.overflow_alphas(oracle, cap)]
    assert deep == [160, 192, 256]


def test_generator_fills_every_cell_under_the_model_and_the_oracle(oracle, batches):
    filled = CC.model_ledger(oracle, batches)
    for group, req in (("main", CC.main_cells()), ("overflow", CC.overflow_cells(oracle)), ("wide", CC.WIDE_CELLS),
                       ("thin", CC.thin_cells())):
        assert CC.missing(req, filled) == [], group
    # every alpha fills most of the main cells by itself (the three calls are not one call's cells split three ways)
    for alpha in CC.ALPHAS:
        sub = [b for b in batches if b.kind == "main" and b.alpha == alpha]
        assert len(CC.missing(CC.main_cells(), CC.model_ledger(oracle, sub))) <= 17, alpha
    assert any((b.q[np.arange(b.stride)[None, :] < b.lens[:, None]] == 0).any() for b in batches)         # some 'N' ...
    assert any((b.q[np.arange(b.stride)[None, :] < b.lens[:, None]] == 255).any() for b in batches)       # ... and 'n'


def test_generator_is_deterministic_and_small(oracle, batches):
    again = CC.generate(oracle, fresh=True)
    assert [b.name for b in again] == [b.name for b in batches]
    for a, b in zip(again, batches):
        assert np.array_equal(a.q, b.q) and np.array_equal(a.lens, b.lens) and a.alpha == b.alpha and a.fixed_len == b.fixed_len
    assert sum(b.n for b in batches) <= MAX_READS
    assert max(b.n for b in batches) <= 4096                 # each also fits the one-read-per-wave entry
    for b in batches:
        assert b.stride % 16 == 0 and b.lens.max() <= b.stride and b.n > 0
        if b.kind == "ovf":
            assert b.fixed_len == b.final_cap - 1 and (b.lens == b.fixed_len).all()


# ---- MPB_FLAG_FAST_FMA and MPB_FLAG_ODDS ---------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def mode_batches(oracle):
    return {mode: CC.generate(oracle, mode=mode) for mode in CC.MODES}


def test_odds_bound_drops_only_far_rows_of_class_1024(oracle):
    """B, the most rows a read can need and still pass ODDS' range guard, is measured on the ladder Q3 .. Q20 (5917 bases
    of Q10 need 693 rows, 62036 of Q20 need 730); the cells beyond it are all in class 1024, none at or below row 688."""
    B = CC.odds_bound(oracle)
    bad = CC.odds_unreachable(oracle)
    assert B >= 693
    assert bad and all(cap == 1024 and js + 1 > B and js > 688 for _, cap, js in bad)
    assert [c for c in CC.main_cells() if c not in bad] == CC.odds_cells(oracle)
    assert all(c[2] + 1 <= B for c in CC.odds_cells(oracle))
    print("ODDS bound B = %d rows; %d cells dropped: rows %s of class 1024" % (B, len(bad), [c[2] for c in bad]))


@pytest.mark.parametrize("mode", CC.MODES)
def test_mode_batches_fill_every_cell_under_the_models(oracle, mode_batches, mode):
    main, thin = CC.model_ledger_mode(oracle, mode_batches[mode], mode)
    if mode == "fma":
        assert CC.missing(CC.main_cells(), main) == [] and CC.missing(CC.thin_cells(), thin) == []
    else:
        assert CC.missing(CC.odds_cells(oracle), main) == []
        assert len(CC.odds_cells(oracle)) + len(CC.odds_unreachable(oracle)) == 170
    # no read of a batch is one the mode hands back at the batch's own alpha and default flags
    for b in mode_batches[mode]:
        assert not oracle.filter_batch_model(b.q, mode, lens=b.lens, alpha=b.alpha, threads=8).hand.any(), b.name


def test_mode_generator_is_deterministic_and_small(oracle, mode_batches):
    total = 0
    for mode in CC.MODES:
        again = CC.generate(oracle, fresh=True, mode=mode)
        assert [b.name for b in again] == [b.name for b in mode_batches[mode]]
        for a, b in zip(again, mode_batches[mode]):
            assert np.array_equal(a.q, b.q) and np.array_equal(a.lens, b.lens) and a.alpha == b.alpha and a.fixed_len is None
            assert b.kind == "main" and b.alpha in CC.MODE_ALPHAS and b.name.startswith(mode + "_")
            assert 0 < b.n <= 4096 and b.stride % 16 == 0 and b.lens.max() <= b.stride
            if b.stride > CC.LONG_STRIDE_MAX:
                assert "far" in b.name and mode == "odds" and b.lens.min() > CC.odds_longest(16) - 300      # Q16 .. Q20 only
        total += sum(b.n for b in again)
    assert total <= MAX_MODE_READS
    for mode in CC.MODES:
        for name, stride, specs, _ in CC.mode_pools(mode):
            if stride > CC.LONG_STRIDE_MAX:
                assert min(s[0] for s in specs) >= 16 and max(s[1] for s in specs) <= 20
                assert sum(len(range(s[2], s[3] + 1, s[4])) for s in specs) <= CC.ODDS_FAR_MAX


@pytest.mark.parametrize("mode", CC.MODES)
def test_equality_with_the_model_proves_the_modes_body_ran(oracle, mode_batches, mode):
    """Per class, some read of the class's ledger has a model (ee, pass) that differs from the exact oracle's: a run that
    equals the model there did not run the exact body.  Class 2 under FMA is the thin one: a read of one base, or one that
    crosses in row 0, has the exact result whatever the arithmetic, and the exact batches' class-2 reads are all of that kind;
    of the ten class-2 reads here one differs (146 bases of Q29 at alpha 0.05, crossing in row 1), and that is asserted."""
    differ = {int(c): 0 for c in CC.CAPS}
    reads = dict(differ)
    for b in mode_batches[mode]:
        exact = oracle.filter_batch(b.q, lens=b.lens, alpha=b.alpha, threads=8)[:3]
        m = oracle.filter_batch_model(b.q, mode, lens=b.lens, alpha=b.alpha, threads=8)
        budgets = CC.cap_of_rows(CC.predicted_rows(b.q, b.lens, b.alpha))
        led = ~m.hand & (budgets > 0) & (m.rows >= 1) & (m.rows <= budgets)
        d = X.differs(exact, m)
        for cap in differ:
            reads[cap] += int((led & (budgets == cap)).sum())
            differ[cap] += int((led & (budgets == cap) & d).sum())
    for cap in differ:
        assert reads[cap] >= 2, cap
        assert differ[cap] >= 1, (cap, reads[cap])
    if mode == "fma":
        assert (differ[2], reads[2]) == (1, 10)
    print("[%s] ledger reads whose model differs from the exact oracle, per class: %s" % (
        mode, {c: "%d/%d" % (differ[c], reads[c]) for c in differ}))


@pytest.mark.parametrize("cap", sorted(CC.GUARD_CORES))
def test_range_guard_ladder_straddles_the_boundary(oracle, cap):
    """Every read of a ladder lies within 0.05 bit of 2^-900, some on each side, consecutive k around the step; the model
    hands back exactly the reads below it, and the predictor puts all of them into class `cap`."""
    q, lens, kc = CC.range_guard_ladder(oracle, cap)
    m = oracle.filter_batch_model(q, "odds", lens=lens, threads=8)
    off = np.log2(m.p0) - CC.P0_MIN_LOG2
    assert (np.abs(off) <= CC.GUARD_BAND).all() and (off > 0).sum() >= 4 and (off < 0).sum() >= 4
    assert np.array_equal(m.hand, m.p0 < 2.0 ** CC.P0_MIN_LOG2) and (np.diff(off) < 0).all()
    step = int(np.argmax(m.hand))
    assert lens[step] - lens[step - 1] == 1 and abs(off[step] - off[step - 1]) < 2e-4
    assert (CC.cap_of_rows(CC.predicted_rows(q, lens, 0.005)) == cap).all() and (m.rows <= cap).all()
    assert (m.rows > CC.prev_cap(cap)).all() and len(lens) <= 16


@pytest.mark.parametrize("mode", CC.MODES)
def test_band_batch_hands_back_inside_1e_9_and_keeps_outside(oracle, mode):
    q, lens = CC.band_batch()
    m0 = oracle.filter_batch_model(q, mode, lens=lens, threads=8, ambigs="ignore")
    assert (CC.cap_of_rows(CC.predicted_rows(q, lens, 0.005)) == 160).all() and not m0.hand.any()
    picks = CC.band_picks(m0)
    assert len(picks) == 3
    for i in picks:
        e = float(m0.ee_model[i])
        for f, inside in CC.BAND_FACTORS:
            for me in (e * (1 - f), e * (1 + f)):
                m = oracle.filter_batch_model(q, mode, lens=lens, threads=8, ambigs="ignore", maxerrors=me)
                assert bool(m.hand[i]) == inside, (i, f, me)


@pytest.mark.parametrize("layout", CC.NARROW_LAYOUTS)
def test_narrow_batches_fill_their_cells(oracle, layout):
    q, lens, fixed = CC.narrow_batch(oracle, layout)
    assert q.shape == (CC.NARROW_N, int(layout[-3:])) and (fixed is None) == layout.startswith("ragged")
    for alpha in (0.005,):
        _, _, _, rows = oracle.filter_batch(q, lens=lens, alpha=alpha, threads=8)
        filled = set()
        for R in (2, 3, 4):
            filled |= CC.ledger_narrow(layout, R, q, lens, rows)
        assert CC.missing([c for c in CC.narrow_cells() if c[1] == layout], filled) == []
    q2, lens2, _ = CC.narrow_batch(oracle, layout)
    assert np.array_equal(q, q2) and np.array_equal(lens, lens2)


def test_predictor_model_never_under_predicts_uniform_reads(oracle):
    """The property the main-pass cells rest on (a read crosses in rows (prev, cap] of its class): on uniform-quality reads the
    model's prediction is never below the oracle's J."""
    rng = np.random.default_rng(3)
    n = 3000
    lens = rng.integers(1, 301, n).astype(np.int32)
    q = np.repeat(rng.integers(1, 42, n).astype(np.uint8)[:, None], 304, 1)
    q[np.arange(304)[None, :] >= lens[:, None]] = 0
    for alpha in CC.ALPHAS:
        _, _, _, rows = oracle.filter_batch(q, lens=lens, alpha=alpha, threads=8)
        assert (rows <= CC.predicted_rows(q, lens, alpha)).all(), alpha
