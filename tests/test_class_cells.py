"""The directed-input generator of tests/helpers/class_cells.py, on the CPU: its class table is the header's, it fills every
required cell under the predictor model and the oracle's rows, it is deterministic and its batches stay small.  (What the GPU
files assert never comes from the model: test_gpu_class_edges.py builds its ledger from the budgets the library reports.)"""
import os

import numpy as np
import pytest

from helpers import class_cells as CC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_READS = 20_000           # all directed batches together: the GPU files run every one of them through several entries


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
