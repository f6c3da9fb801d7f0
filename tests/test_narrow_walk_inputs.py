"""The directed inputs of tests/helpers/narrow_walk.py for the multi-block walk of the narrow pass, on the CPU: the instance table is
the dispatch the kernel source states, the plan arithmetic gives the hand-computed walks and segment starts, and under the oracle's
rows (the odds model's for the twins) every required cell of every instance is filled on both capped grids.  A failure of
tests/test_gpu_narrow_walk.py is then the kernel's, not the input's."""
import os
import time

import numpy as np
import pytest

from helpers import narrow_walk as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "moira_amd", "csrc")


@pytest.fixture(scope="module")
def parsed():
    return W.parse_sources(open(os.path.join(CSRC, "mpb_kernels.hip")).read(), open(os.path.join(CSRC, "mpb_internal.h")).read())


def test_the_instance_table_is_the_dispatch(parsed):
    P = parsed
    assert (P["chunk"], P["max_stride_log2"], P["half"], P["only_rows"], P["line"]) == (16, 16, 64, 2, 128)
    assert P["max_stride"] == 1 << P["max_stride_log2"]                  # no accepted stride is refused by nar_rs_reads_per_lane
    assert P["index_text"]                                                # the lines that index the tables: as dispatch() restates them
    assert sorted(P["tables"]) == ["k_narrow", "k_narrow_rg", "k_narrow_rs", "k_odds_nar", "k_odds_nar_rg", "k_odds_nar_rs"]
    assert P["tables"]["k_narrow_rs"] == ["k_narrow_rs<2, true>", "k_narrow_rs<3, true>", "k_narrow_rs<4, true>", "k_narrow_rs<2, false>"]
    assert P["tables"]["k_narrow_rg"] == ["k_narrow_rg<2, 2>", "k_narrow_rg<3, 3>", "k_narrow_rg<4, 4>", "k_narrow_rg<3, 2>", "k_narrow_rg<4, 3>"]
    for exact, odds in (("k_narrow", "k_odds_nar"), ("k_narrow_rs", "k_odds_nar_rs")):
        assert [k.replace(exact, odds) for k in P["tables"][exact]] == P["tables"][odds]
    assert P["tables"]["k_odds_nar_rg"] == ["k_odds_nar_rg<2>", "k_odds_nar_rg<3>", "k_odds_nar_rg<4>"]
    assert len(W.INSTANCES) == 28 and len(set(W.INSTANCES)) == 28 and len({W.name_of(i) for i in W.INSTANCES}) == 28
    assert sum(i.odds for i in W.INSTANCES) == 13
    # what calls can launch is what the table lists ...
    assert W.reachable(P) == {W.instance_key(i) for i in W.INSTANCES}
    # ... each instance at each of its shapes
    for inst in W.INSTANCES:
        for shape in W.shapes_of(inst):
            if inst.family == "rg":
                got = W.dispatch(P, shape[2], inst.R, True, shape[3] if inst.RLO < inst.R else 0, inst.odds)
                assert shape[2] <= P["rg_max_stride"] and 1 <= shape[3] <= 255
            else:
                assert shape[0] <= shape[1]
                got = W.dispatch(P, shape[1], inst.R, False, 0, inst.odds)
            assert got == W.instance_key(inst), (inst, shape)
    # the stride conditions of the table
    for inst in W.INSTANCES:
        for shape in W.shapes_of(inst):
            s = shape[1] if inst.family != "rg" else shape[2]
            if inst.family == "ring": assert s % 64 != 0
            if inst.family == "rs": assert {1: s % 128 == 0, 2: s % 128 == 64, 4: s % 64 == 32, 8: s % 32 == 16}[inst.k]
    assert [W.key_shift_of(s[2], P["rg_bins"]) for s in W.RAGGED_SHAPES] == [0, 0, 0, 3]
    assert (P["rg_win"], W.GROUP, P["ring_depth"]) == (W.RG_WIN, 64, 2)


def test_the_unreachable_kernels_are_pinned(parsed):
    held = {k for names in parsed["tables"].values() for k in names}
    assert len(held) == 22
    assert held - {k for k, _ in W.reachable(parsed)} == set(W.UNREACHABLE) == {"k_narrow<2, MPB_NAR_DEPTH>", "k_odds_nar<2, MPB_NAR_DEPTH>"}
    assert all(len(reason) > 40 for reason in W.UNREACHABLE.values())
    # the reason: two rows never leave k_narrow_rs
    ks = {W.rs_reads_per_lane(parsed, s, 2) for s in range(16, parsed["max_stride"] + 1, 16)}
    assert ks == {1, 2, 4, 8}
    assert W.rs_reads_per_lane(parsed, 304, 3) == 0 and W.rs_reads_per_lane(parsed, 320, 3) == 2


def test_the_plan_arithmetic(parsed):
    assert parsed["grid_lines"] == W.GRID_LINES                           # the one copy of the grid sizing, as grid_blocks() restates it
    assert parsed["cap_max"] == parsed["max_waves"] // 4 == 2048
    # 29 blocks on the three grids
    assert [W.grid_blocks(29, c) for c in (1, 3, None)] == [1, 3, 8]
    assert W.walk(0, 29, 4) == [0, 4, 8, 12, 16, 20, 24, 28] and W.walk(1, 29, 4) == [1, 5, 9, 13, 17, 21, 25]
    assert [len(W.walk(g, 29, 4)) for g in range(4)] == [8, 7, 7, 7] and 29 % 4 == 1
    assert [len(W.walk(g, 29, 12)) for g in range(12)] == [3] * 5 + [2] * 7 and 29 % 12 == 5
    assert W.walk(4, 29, 12) == [4, 16, 28] and W.walk(5, 29, 12) == [5, 17]
    assert [len(W.walk(g, 29, 32)) for g in range(32)] == [1] * 29 + [0] * 3
    # segment starts: per_blk x (blocks owned by the waves before)
    assert [W.seg_start(g, 29, 4, 64) for g in range(4)] == [0, 512, 960, 1408]
    assert [W.seg_start(g, 29, 12, 128) for g in range(7)] == [0, 384, 768, 1152, 1536, 1920, 2176]
    assert [W.seg_start(g, 29, 32, 512) for g in (0, 1, 28, 29, 31)] == [0, 512, 28 * 512, 29 * 512, 29 * 512]
    for nblk, Wv, per_blk in ((29, 4, 64), (29, 12, 512), (29, 32, 128), (7, 4, 64), (8, 4, 256)):
        owned = 0
        for g in range(Wv):
            assert W.seg_start(g, nblk, Wv, per_blk) == per_blk * owned
            owned += len(W.walk(g, nblk, Wv))
        assert owned == nblk
    # the batches: n = 29 per_blk - 37; the last block is partial, and with two reads per lane the last read is a lane's first
    assert [W.fixed_n(64 * k) for k in (1, 2, 4, 8)] == [1819, 3675, 7387, 14811]
    assert all((W.fixed_n(64 * k) + 64 * k - 1) // (64 * k) == 29 for k in (1, 2, 4, 8))
    assert (W.fixed_n(128) - 1 - 28 * 128) % 2 == 0
    # the workspace: the segments of any W end at per_blk * nblk <= n + per_blk - 1, inside nar_seg's n + n / 8 + 1024 + 64 entries
    for k in (1, 2, 4, 8):
        n = W.fixed_n(64 * k)
        assert W.seg_start(4, 29, 4, 64 * k) == 29 * 64 * k <= n + 64 * k - 1 < n + n // 8 + 1024 + 64
    # ragged: five windows, 272 groups, the last of 40 reads; cap1 has three cuts for four interior borders
    n = W.RAGGED_N
    assert (n, n % 64, (n + 4095) // 4096, (n + 63) // 64) == (17384, 40, 5, 272)
    assert [4 * W.grid_blocks(272, c) for c in (1, 3, None)] == [4, 12, 272]
    inst = [i for i in W.INSTANCES if i.family == "rs" and i.k == 8][0]
    assert [W.expected_waves(inst, 14811, g) for g in ("cap1", "cap3", "control")] == [4, 12, 32]


def test_the_sort_model():
    lens = np.array([40, 0, 16, 17, 300, 1, 16], np.int32)
    assert W.rag_order(lens, 0).tolist() == [1, 2, 5, 6, 3, 0, 4]        # keys 3 0 1 2 19 1 1: stable
    assert W.rag_order(lens, 3).tolist() == [0, 1, 2, 3, 5, 6, 4]        # keys 0 0 0 0 2 0 0
    rng = np.random.default_rng(1)
    lens = rng.integers(0, 301, 4096 + 200).astype(np.int32)
    G = W.Groups(lens, 0)
    assert sorted(G.order[:4096].tolist()) == list(range(4096)) and sorted(G.order[4096:].tolist()) == list(range(4096, 4296))
    key = (lens[G.order] + 15) >> 4
    assert (np.diff(key[:4096]) >= 0).all() and (np.diff(key[4096:]) >= 0).all()
    assert G.ngroups == 68 and G.size[-1] == 8 and (G.full <= G.maxc).all()
    assert G.maxc[0] == key[63] and G.panels.min() >= 1


@pytest.fixture(scope="module")
def fixed(oracle):
    t = time.time()
    out = {(L, s, k): W.fixed_batch(oracle, L, s, k) for (fam, k), shapes in W.FIXED_SHAPES.items() for L, s in shapes for k in [k or 1]}
    print("fixed-length batches: %d, %d reads, %.1f s" % (len(out), sum(b.n for b in out.values()), time.time() - t))
    return out


@pytest.fixture(scope="module")
def ragged(oracle):
    t = time.time()
    out = {s: W.ragged_batch(oracle, *s[:3]) for s in W.RAGGED_SHAPES}
    print("ragged batches: %d of %d reads, %.1f s" % (len(out), W.RAGGED_N, time.time() - t))
    return out


def test_every_fixed_cell_is_filled(fixed):
    missing, count = [], 0
    for inst in W.INSTANCES:
        if inst.family == "rg":
            continue
        for L, stride in W.shapes_of(inst):
            b = fixed[(L, stride, inst.k or 1)]
            assert (b.n, b.q.shape) == (W.fixed_n(W.per_block(inst)), (b.n, stride))
            req = W.required_fixed(inst, L)
            for grid in W.CAPPED:
                got = W.fixed_ledger(inst, b, grid)
                missing += [(W.name_of(inst), L, stride, grid, c) for c in sorted(req - got, key=str)]
                count += len(req)
            assert W.fixed_ledger(inst, b, "control") == set()           # one block per wave: nothing of the walk
    assert missing == [], missing[:20]
    print("required cells of the fixed-length instances, both grids: %d" % count)


def test_what_short_reads_cannot_have():
    """A read of L bases has L + 1 rows: the one-base shape asks for J = 1, 2 only (its hand-backs are 'n' bytes)."""
    two = [i for i in W.INSTANCES if i.family == "rs" and i.k == 8 and not i.odds][0]
    assert W.rows_that_exist(two, 1) == [1, 2] and W.rows_that_exist(two, 16) == [1, 2, 3]
    four = [i for i in W.INSTANCES if i.family == "ring" and i.R == 4 and not i.odds][0]
    assert W.rows_that_exist(four, 17) == [1, 2, 3, 4, 5]
    assert ("phase", 1) in W.required_fixed(four, 300) and ("phase", 1) not in W.required_fixed(four, 100)
    assert len(W.required_fixed(four, 300)) == 15 + 6 + 2 + 2
    pair = [i for i in W.INSTANCES if i.family == "rs" and i.k == 2 and i.R == 3 and i.odds][0]
    assert set(W.PAIR_CELLS) <= W.required_fixed(pair, 300) and not W.pair_stores(pair._replace(R=4))


def test_the_fixed_batches_are_what_they_say(fixed):
    for (L, stride, k), b in fixed.items():
        assert b.lens.tolist() == [L] * b.n and not b.q.flags.writeable
        assert b.patterns[-1] == "mixed" and b.n % 2 == 1
        exact2 = [i for i in W.INSTANCES if i.family == "rs" and i.R == 2 and i.k == 8 and not i.odds][0]
        for R in (2, 3, 4):
            for odds in (False, True):
                h = b.handed(exact2._replace(R=R, RLO=R, odds=odds))
                for blk, p in enumerate(b.patterns):                      # the drawn patterns hold for every row count and both arithmetics
                    if p != "mixed":
                        assert W.block_pattern(h, blk, b.per_blk, b.n) == p, (L, stride, k, R, odds, blk)
                assert not h[-1]
        assert 0.2 < b.handed(exact2).mean() < 0.9
        # the reads are not uniform: a read's bases differ, and so do the reads
        if L >= 16:
            assert (b.q[:, :L].max(1) > b.q[:, :L].min(1)).mean() > 0.9
    assert len(fixed) == 20


def test_every_ragged_cell_is_filled(ragged):
    missing = []
    for inst in W.INSTANCES:
        if inst.family != "rg":
            continue
        for shape in W.shapes_of(inst):
            b = ragged[shape]
            assert b.lens.min() >= 0 and b.lens.max() <= shape[2] and b.lens.min() == shape[0] and b.lens.max() == shape[1]
            for grid in W.CAPPED:
                req = W.required_ragged(inst, shape, grid)
                got = W.ragged_ledger(inst, b, shape, grid)
                missing += [(W.name_of(inst), shape, grid, c) for c in sorted(req - got, key=str)]
    assert missing == [], missing[:20]
    three = [i for i in W.INSTANCES if i.family == "rg" and i.RLO == 2 and i.R == 3][0]
    assert W.required_ragged(three, W.RAGGED_SHAPES[0], "cap1") == {("window_border",), ("straddle",), ("all_next_to_none",),
                                                                     ("partial_last_group",), ("len0_group",), ("split_both",), ("rows_change",)}
    assert W.required_ragged(three, W.RAGGED_SHAPES[3], "cap3") == set() and W.required_ragged(three, W.RAGGED_SHAPES[3], "cap1") == {("window_border",)}
    assert ("len0_group",) not in W.required_ragged(three, W.RAGGED_SHAPES[1], "cap1")


def test_the_generator_is_deterministic(oracle, fixed, ragged):
    b = fixed[(17, 48, 1)]
    again = W._fixed_batch(oracle, 17, 48, 1)
    assert np.array_equal(again.q, b.q) and again.patterns == b.patterns
    r = ragged[W.RAGGED_SHAPES[0]]
    again = W._ragged_batch(oracle, *W.RAGGED_SHAPES[0][:3])
    assert np.array_equal(again.q, r.q) and np.array_equal(again.lens, r.lens) and len(r.planted) == W.PAIRS_PLANTED
