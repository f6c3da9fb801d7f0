"""The directed k_wide inputs of tests/helpers/wide_cells.py, on the CPU: the constants and the instance filter are the kernel
source's, the committed length table reproduces its J under the oracle, the generator fills every required cell under the
oracle's rows and the float64 model, it is deterministic and small, and the list batch meets the conditions its GPU tests rest
on.  (What the GPU file asserts is the oracle's result; the model only says what a batch claims to cover.)"""
import os
import re
import time

import numpy as np
import pytest

from helpers import wide_cells as WC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "moira_amd", "csrc")


@pytest.fixture(scope="module")
def batches():
    return WC.generate()


@pytest.fixture(scope="module")
def results(oracle, batches):
    t = time.time()
    out = {b.name: WC.oracle_results(oracle, b) for b in batches}
    print("oracle, directed batches, 8 threads: %.1f s" % (time.time() - t))
    return out


@pytest.fixture(scope="module")
def list_rows(oracle):
    t = time.time()
    b = WC.list_batch()
    ee, _, _, rows = oracle.filter_batch(b.q, lens=b.lens, alpha=b.alpha, threads=8)
    print("oracle, list batch, 8 threads: %.1f s" % (time.time() - t))
    return ee, rows


def test_constants_and_the_instance_filter_are_the_sources():
    kern = open(os.path.join(CSRC, "mpb_kernels.hip")).read()
    head = open(os.path.join(CSRC, "mpb_internal.h")).read()
    define = lambda text, name: int(re.search(r"#define\s+%s\s+(\d+)\s" % name, text).group(1))
    assert define(head, "MPB_WIDE_WAVES") == WC.WIDE_WAVES == 16
    assert define(kern, "MPB_WIDE_R") == WC.WIDE_R == 16
    assert define(kern, "MPB_WIDE_GRID") == WC.WIDE_GRID == 1024
    assert define(head, "MPB_TILE_MAX_ROWS") == WC.WAVE_ROWS == 64 * WC.WIDE_R
    # the filter, the wave count and the list loop as the kernel states them
    assert "if (nw > W || (W > 2 && nw <= W / 2)) continue;" in kern
    assert "const int nw = max(1, min(MPB_WIDE_WAVES, (rows + 64 * R - 1) / (64 * R)));" in kern
    assert "for (int k = blockIdx.x; k < nlist; k += gridDim.x) {" in kern
    assert "const int rows = FINAL ? li + 1 : gload(budget + k);" in kern
    # the instances that are launched: W = 2 always, 4 / 8 / 16 by the batch's longest row
    got = [int(w) for w in re.findall(r"hipLaunchKernelGGL\(\(k_wide<FINAL, (\d+)>\), dim3\(MPB_WIDE_GRID\), dim3\(64 \* \1\)", kern)]
    assert got == list(WC.INSTANCES)
    assert [int(w) for w in re.findall(r"if \(max_waves > (\d+)\) hipLaunchKernelGGL\(\(k_wide", kern)] == [2, 4, 8]
    # W_of restates the filter: every wave count is taken by exactly one instance, the one W_of names
    for nw in range(1, WC.WIDE_WAVES + 1):
        takers = [W for W in WC.INSTANCES if WC.kernel_takes(W, nw)]
        assert takers == [WC.W_of(nw)], nw
    assert [WC.W_of(nw) for nw in (1, 2, 3, 4, 5, 8, 9, 16)] == [2, 2, 4, 4, 8, 8, 16, 16]
    assert list(WC.nw_of([1, 1024, 1025, 2048, 2049, 16384, 16385, 70000])) == [1, 1, 2, 2, 3, 16, 16, 16]


def test_required_cells():
    req = WC.required_cells()
    assert len(req) == len(set(req)) == 86 and len(WC.trips_cells()) == 2
    assert all(WC.group_of(c) in WC.GROUPS for c in req + WC.trips_cells())
    assert ("wide", "main", 15, "first") in req and ("wide", "final", 15, "last") in req and ("wide", "main", 16, "last") in req
    assert set(WC.ladder_targets(WC.ALPHA)) >= {1024 * w + d for w in range(1, 16) for d in (0, 1)} | {16384, 16385, 2047, 4095, 8191}
    assert WC.ladder_targets(WC.ALPHA_B) == [1024 * w + d for w in range(1, 5) for d in (0, 1)][1:]


def test_the_length_table_reproduces_its_rows(oracle, batches, results):
    """Every (alpha, J) -> (bases, k, tail) of LADDER: the oracle needs J rows for that read, and the model is sure of its row count
    and calls it wide.  (The reads are those of the directed batches: their rows are computed once.)"""
    for alpha in (WC.ALPHA, WC.ALPHA_B):
        assert sorted(j for a, j in WC.LADDER if a == alpha) == WC.ladder_targets(alpha)
    seen = 0
    for b in batches:
        rows = results[b.name][3]
        m = WC.Rows(b.q, b.lens, b.alpha)
        for (alpha, J), (L, k, tail) in WC.LADDER.items():
            if alpha != b.alpha:
                continue
            row = WC.ladder_read(L, k, tail)
            at = [i for i in np.nonzero(b.lens == L + tail)[0] if np.array_equal(b.q[i, :L + tail], row)]
            for i in at:
                assert rows[i] == J and m.sure_rows[i] and m.lo[i] > WC.WAVE_ROWS, (alpha, J, L, k, tail, int(rows[i]))
                assert m.rows[i] in (J, J + 1)
                seen += 1
    assert seen == len(WC.LADDER)


def test_search_reproduces_a_table_entry(oracle):
    """The search that made the table, on its cheapest windows (the first two wave boundaries)."""
    got = WC.search_ladder(oracle, WC.ALPHA, targets=[1024, 1025, 2047, 2048, 2049])
    assert got == {j: WC.LADDER[(WC.ALPHA, j)] for j in (1024, 1025, 2047, 2048, 2049)}
    got = WC.search_ladder(oracle, WC.ALPHA_B, targets=[1024, 1025])
    assert got == {1025: WC.LADDER[(WC.ALPHA_B, 1025)]}              # no surely wide read of J = 1024 at this alpha (see LADDER)


def test_generator_fills_every_cell_under_the_model_and_the_oracle(batches, results):
    filled = set()
    for b in batches:
        ee, _, _, rows = results[b.name]
        filled |= WC.ledger(b, rows, nan=np.isnan(ee))
    filled = WC.fold(filled)
    assert WC.missing(WC.required_cells(), filled) == []
    # the second alpha fills the boundaries of the first four waves by itself
    b = [b for b in batches if b.alpha == WC.ALPHA_B][0]
    own = WC.ledger(b, results[b.name][3])
    assert WC.missing([c for c in WC.boundary_cells("main") + WC.boundary_cells("final") if c[2] <= 3 and c[2:] != (1, "last")], own) == []
    count = {g: sum(1 for c in WC.required_cells() if WC.group_of(c) == g) for g in WC.GROUPS}
    print("required cells per group, all filled: %s" % count)
    # the read beyond the range has no supported result: more rows than sixteen waves hold
    big = [b for b in batches if b.stride == WC.STRIDES[-1]][0]
    assert (results[big.name][3] == WC.MAX_ROWS + 1).sum() == 1 and results[big.name][3].max() == WC.MAX_ROWS + 1


def test_generator_is_deterministic_and_small(batches, results):
    again = WC.generate(fresh=True)
    assert [b.name for b in again] == [b.name for b in batches]
    for a, b in zip(again, batches):
        assert np.array_equal(a.q, b.q) and np.array_equal(a.lens, b.lens) and a.alpha == b.alpha and a.fixed_len is None
    assert sum(b.n for b in batches) <= 400
    assert sum(int((results[b.name][3] > 8192).sum()) for b in batches) <= 40
    for b in batches:
        assert b.stride % 16 == 0 and b.stride > 1023 and b.lens.max() <= b.stride and b.n > 0
        dead = np.arange(b.stride)[None, :] >= b.lens[:, None]
        assert (b.q[dead] == 0).any() and (b.q[dead] == 255).any() and len(np.unique(b.q[dead])) == 256      # garbage behind the reads


def test_small_part_holds_the_first_four_waves(batches, results):
    """The sub-batch the modes and the other arithmetics run: every read of at most 4096 rows, the ambiguity reads among them."""
    b = batches[0]
    sub, keep = WC.small_part(b, results[b.name][3])
    rows = results[b.name][3][keep]
    assert rows.max() == 4096 and {1024, 1025, 2048, 2049, 3072, 3073} <= set(int(r) for r in rows)
    filled = WC.ledger(sub, rows)
    assert {("wide", p, what) for p in WC.PASSES for what in ("N_run", "N_last", "n")} <= filled
    assert (sub.lens == 0).sum() == 1


def test_list_batch_conditions(list_rows):
    b = WC.list_batch()
    ee, rows = list_rows
    long_ = b.group <= 1
    assert long_.sum() >= WC.TRIPS_MIN and (b.group == 2).sum() >= 200 and b.stride % 16 == 0 and b.stride > 1023
    assert len(np.unique(b.q[long_], axis=0)) == long_.sum()                          # all different
    live = np.arange(b.stride)[None, :] < b.lens[:, None]
    share0 = (b.q[long_] == 0)[live[long_]].mean()
    assert 0.005 < share0 < 0.015 and 0 < (b.q[long_] == 255)[live[long_]].sum() < 0.001 * live[long_].sum()
    assert not np.isnan(ee).any() and (rows[long_] > WC.WAVE_ROWS).all() and (b.lens == 0).sum() == 1
    plain, under = WC.list_expect(b, rows)                                             # asserts the conditions on every read
    assert plain == 0 and under >= WC.TRIPS_MIN
    assert WC.ledger_trips(b, rows) == set(WC.trips_cells())
    # the two groups alternate: no run of one group in the batch's order is long enough to fill a trip of the grid
    g = b.group[long_]
    runs = np.diff(np.r_[0, np.nonzero(np.diff(g))[0] + 1, len(g)])
    assert runs.max() < 64
    again = WC._CACHE.pop("list")
    fresh = WC.list_batch()
    assert np.array_equal(again.q, fresh.q) and np.array_equal(again.lens, fresh.lens)
