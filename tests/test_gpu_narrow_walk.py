"""The multi-block walk of the natural-order narrow pass on the GPU: every kernel instance the entry can reach (k_narrow,
k_narrow_rs, k_narrow_rg and the one-FMA twins; tests/helpers/narrow_walk.py lists them) on batches of a few thousand reads, with
the persistent grid capped by MPB_NARROW_GRID_BLOCKS (include/moira_pb.h) so that a wave walks block after block, prefetches
across block borders, keeps one hand-back segment over several blocks and k_nar_compact reads the segments of waves that own
different numbers of blocks.  Per instance and shape one resident batch runs on three grids: one workgroup (4 waves), three
(12 waves) and the library's own (a wave per block, the control).

Every comparison is bit for bit and leaves no read out: the exact instances against the oracle (finished reads and the reads
handed back through the sorted pipeline alike), the twins by the rule of tests/helpers/odds_forced.py against the CPU model of the
one-FMA arithmetic; mpb_path_info.narrow_waves says that the cap applied, n_fallback that exactly the reads the ledger calls handed
back were; the three grids' result arrays are byte-identical.  tests/test_narrow_walk_inputs.py shows on the CPU that the batches
fill every cell of the walk."""
import numpy as np
import pytest

from helpers import narrow_walk as W
from helpers.device_runs import Resident
from helpers.odds_forced import check_forced_results

pytestmark = pytest.mark.gpu

HOOK = "MPB_NARROW_GRID_BLOCKS"


@pytest.fixture(scope="module")
def eng():
    from moira_amd.engine import Engine
    e = Engine(0)
    e.batched_only = True
    yield e
    e.close()


def bits(got):
    ee, ns, ps = got
    return ee.view(np.uint64).tobytes(), ns.tobytes(), ps.tobytes()


def walk_check(eng, monkeypatch, inst, batch, split=0, handed=None, res_offset=0):
    """The batch through the instance on the three grids: every assertion of the module's text."""
    q, lens, n, R = batch.q, batch.lens, batch.n, inst.R
    ex_ee, ex_ns, ex_ps = batch.ex
    handed = batch.handed(inst) if handed is None else handed
    kw = dict(narrow_rows=R)
    if inst.odds:
        kw.update(odds=True, odds_narrow=True)
    if split:
        kw.update(narrow_split=split)
    res = Resident(eng, q, lens if batch.ragged else None, res_offset=res_offset)
    seen = {}
    try:
        for grid, cap in W.GRIDS.items():
            if cap is None:
                monkeypatch.delenv(HOOK, raising=False)
            else:
                monkeypatch.setenv(HOOK, str(cap))
            ee, ns, ps, c, path, intact = res.run(fixed_len=None if batch.ragged else batch.L, **kw)
            assert intact, grid
            assert path["narrow_rows"] == R and path["narrow_split"] == split, (grid, path)
            assert path["narrow_waves"] == W.expected_waves(inst, n, grid), (grid, path["narrow_waves"])
            if inst.odds:
                check_forced_results((ee, ns, ps), c, path, q, lens, R, batch.ex, batch.m)
            else:
                bad = np.flatnonzero(~(((ee == ex_ee) | (np.isnan(ee) & np.isnan(ex_ee))) & (ns == ex_ns) & (ps == ex_ps)))
                assert bad.size == 0, "%s: %d reads differ from the oracle, first %s (blocks %s): got %r want %r" % (
                    grid, bad.size, bad[:5].tolist(), (bad[:5] // W.per_block(inst)).tolist(), ee[bad[:5]].tolist(), ex_ee[bad[:5]].tolist())
                assert (c.n_reads, c.n_pass, c.n_fail) == (n, int(ex_ps.sum()), n - int(ex_ps.sum())), grid
            assert path["n_fallback"] == int(handed.sum()), (grid, path["n_fallback"], int(handed.sum()))
            seen[grid] = bits((ee, ns, ps))
    finally:
        monkeypatch.delenv(HOOK, raising=False)
        res.free()
    assert seen["cap1"] == seen["control"] and seen["cap3"] == seen["control"]


FIXED = [(inst, L, stride) for inst in W.INSTANCES if inst.family != "rg" for L, stride in W.shapes_of(inst)]
RAGGED = [(inst, shape) for inst in W.INSTANCES if inst.family == "rg" for shape in W.shapes_of(inst)]


@pytest.mark.parametrize("inst,L,stride", FIXED, ids=["%s-%d-%d" % (W.name_of(i), L, s) for i, L, s in FIXED])
def test_fixed_length_walk(eng, oracle, monkeypatch, inst, L, stride):
    batch = W.fixed_batch(oracle, L, stride, inst.k or 1)
    walk_check(eng, monkeypatch, inst, batch)
    if W.pair_stores(inst):
        # two reads per lane, R <= 3: result arrays an element off their alignment take the single stores
        walk_check(eng, monkeypatch, inst, batch, res_offset=1)


@pytest.mark.parametrize("inst,shape", RAGGED, ids=["%s-%d_%d-%d" % ((W.name_of(i),) + s[:3]) for i, s in RAGGED])
def test_ragged_walk(eng, oracle, monkeypatch, inst, shape):
    batch = W.ragged_batch(oracle, *shape[:3])
    mixed = inst.RLO < inst.R
    split = shape[3] if mixed else 0
    handed = batch.handed(inst, W.rows_allowed(inst, batch.groups, split)) if mixed else None
    walk_check(eng, monkeypatch, inst, batch, split=split, handed=handed)


def test_values_the_hook_ignores(eng, oracle, monkeypatch):
    """Unset, empty, 0, negative, above 2048 or not a number: today's grid."""
    inst = [i for i in W.INSTANCES if i.family == "rs" and i.k == 2 and i.R == 2 and not i.odds][0]
    batch = W.fixed_batch(oracle, 300, 320, 2)
    res = Resident(eng, batch.q)
    try:
        for value, waves in ((None, 32), ("", 32), ("0", 32), ("-1", 32), ("2049", 32), ("3x", 32), ("2048", 32), ("2", 8), ("1", 4)):
            if value is None:
                monkeypatch.delenv(HOOK, raising=False)
            else:
                monkeypatch.setenv(HOOK, value)
            ee, ns, ps, c, path, intact = res.run(fixed_len=300, narrow_rows=2)
            assert intact and path["narrow_waves"] == waves, (value, path)
            assert np.array_equal(ee, batch.ex[0], equal_nan=True) and np.array_equal(ps, batch.ex[2])
            ee, ns, ps, c, path, intact = res.run(fixed_len=300, no_narrow=True)
            assert path["narrow_waves"] == 0 and path["narrow_rows"] == 0
    finally:
        monkeypatch.delenv(HOOK, raising=False)
        res.free()
    assert W.expected_waves(inst, batch.n, "control") == 32
