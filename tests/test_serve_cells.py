"""The directed inputs of tests/helpers/serve_cells.py for the resident per-read kernel, on the CPU: the constants are the kernel
source's, the generator is deterministic and small, every stated cell is filled under the oracle's rows and the float64 model (or
is listed as unreachable, with its reason), no kept read is unsure, and the packed form of a read gives the per-read entry's
expectation.  (What the GPU file asserts is the oracle's result; the model only says what the set claims to cover.)"""
import os
import time

import numpy as np
import pytest

from helpers import class_cells as CC
from helpers import serve_cells as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "moira_amd", "csrc")


@pytest.fixture(scope="module")
def batches(oracle):
    t = time.time()
    out = SC.generate(oracle)
    print("generator: %.1f s" % (time.time() - t))
    return out


@pytest.fixture(scope="module")
def results(oracle, batches):
    t = time.time()
    out = [SC.oracle_results(oracle, b) for b in batches]
    print("oracle, %d directed reads, 8 threads: %.2f s" % (sum(b.n for b in batches), time.time() - t))
    return out


def test_constants_are_the_sources():
    kern = open(os.path.join(CSRC, "mpb_kernels.hip")).read()
    head = open(os.path.join(CSRC, "mpb_internal.h")).read()
    got = SC.parse_sources(kern, head)
    assert got == {"reg_max_bases": SC.REG_MAX_BASES, "reg_max_rows": SC.REG_MAX_ROWS, "chunk": SC.CHUNK, "chunk_round": SC.CHUNK - 1,
                   "cdf_rows": SC.REG_MAX_ROWS, "serve_stride": SC.SERVE_STRIDE, "small_max_stride": SC.SMALL_MAX_STRIDE,
                   "tile_max_rows": CC.TILE_MAX_ROWS}
    assert (SC.REG_MAX_BASES, SC.REG_MAX_ROWS, SC.SERVE_STRIDE, SC.CHUNK) == (1024, 64, 2048, 16)
    assert SC.REG_MAX_BASES == 64 * SC.CHUNK                     # one chunk per lane
    # the hosts post a read of at most MPB_SERVE_STRIDE - 1 bases, and only one without a private table
    for name in ("mpb_perread.cpp", "mpb_broker.cpp"):
        assert "len <= MPB_SERVE_STRIDE - 1" in open(os.path.join(CSRC, name)).read(), name
    # the thin body of a prediction, as the kernel picks it and as tcap() restates it
    assert "const int thin = rows <= 2 ? 0 : 31 - __builtin_clz(rows - 1);" in kern
    thin_caps = [c[0] for c in CC.THIN_CLASSES]
    for rows in (1, 2, 3, 4, 5, 8, 9, 64, 65, 128, 129, 1023, 1024):
        thin = 0 if rows <= 2 else (rows - 1).bit_length() - 1
        assert thin_caps[thin] == int(SC.tcap(rows)) == int(CC.thin_cap_of_budget(CC.cap_of_rows(rows))), rows


def test_required_cells():
    req = SC.required()
    count = {g: sum(1 for c in req if SC.group_of(c) == g) for g in SC.GROUPS}
    assert count == {"js": 64, "chunks": 4, "tail": 48, "under": 5, "below": 5, "J65": 1, "amb": 7, "gate": 8, "sthin": 28}
    assert sum(count.values()) == len(req)
    assert req[("reg", "js", 63)] == SC.ALPHAS and req[("reg", "js", 40)] == SC.ALPHAS[:1]
    assert {c for c in req if c[0] == "sthin"} == {("sthin",) + c[1:] for c in CC.thin_cells()}
    assert set(SC.UNREACHABLE) <= set(req)


def test_the_unreachable_cells_are_pinned(batches, results):
    """One cell: no read of J in 49 .. 64 has a prediction whose thin cap lies below J (that takes a prediction 17 rows short).  The
    reads whose prediction alone is short reach every bin (("reg", "below", k)), and the largest J of an `under` read is 33 .. 36."""
    assert list(SC.UNREACHABLE) == [("reg", "under", 4)]
    assert all(len(reason) > 40 for reason in SC.UNREACHABLE.values())
    under = []
    for b, (ee, _, _, rows) in zip(batches, results):
        under += [int(rows[i]) for i in range(b.n) if not b.pred.amb[i] and b.pred.body()[i] == "reg" and b.pred.cap_hi[i] < rows[i] <= 64]
    assert len(under) >= 8 and min(under) < 8 and 32 < max(under) <= 36, sorted(under)


def test_every_cell_is_filled_or_listed_as_unreachable(oracle, batches):
    filled = SC.ledger_all(oracle, batches)
    assert SC.missing(filled) == []
    assert not any(c in SC.UNREACHABLE for c, _ in filled)      # a cell that a read reaches after all leaves the list
    count = {g: len({c for c, _ in filled if SC.group_of(c) == g and c in SC.required()}) for g in SC.GROUPS}
    print("cells filled per group: %s" % count)


def test_no_kept_read_is_unsure(batches, results):
    for b, (ee, _, _, rows) in zip(batches, results):
        assert not np.isnan(ee).any(), b.name                   # every read has a result: none is left to the `no crossing` rule
        assert b.pred.sure_with(rows).all(), b.name
        assert b.stride == SC.STRIDE and b.lens.max() <= SC.SERVE_STRIDE
        dead = np.arange(b.stride)[None, :] >= b.lens[:, None]
        assert (b.q[dead] == 0).all()
        # the ambiguous reads: the prediction cannot matter
        amb = b.pred.amb
        assert (rows[amb] <= 2).all() and (b.lens[amb] <= SC.REG_MAX_BASES).all()


def test_generator_is_deterministic_and_small(oracle, batches):
    again = SC.generate(oracle, fresh=True)
    assert [b.alpha for b in again] == [b.alpha for b in batches] == sorted(SC.ALPHAS + SC.DEEP_ALPHAS, reverse=True)
    for a, b in zip(again, batches):
        assert np.array_equal(a.q, b.q) and np.array_equal(a.lens, b.lens)
    n = sum(b.n for b in batches) + len(SC.PRIV)
    print("generated reads: %d" % n)
    assert 300 <= n <= SC.MAX_READS == 1500
    for b in batches:
        assert len({b.q[i].tobytes() + bytes([b.lens[i] & 255, b.lens[i] >> 8]) for i in range(b.n)}) == b.n     # all different


def test_packed_rows_state_the_per_read_calls(oracle, batches, results):
    """The two forms of a read agree: the oracle's per-read entry on (seq, quals, alpha) gives what one oracle call per alpha
    gives on the packed matrix (ambiguous bases counted, never added; no limit)."""
    want = SC.expected(oracle, batches)
    calls = SC.calls(batches)
    assert len(calls) == len(want) == sum(b.n for b in batches) + len(SC.PRIV)
    for key, seq, quals, alpha in calls:
        assert oracle.ee_rowwise(seq, quals, alpha)[:2] == want[key], key
    assert all(max(q) > 254 for _, q, _ in SC.PRIV)


def test_handed_back_reads_and_sequences(oracle, batches, results):
    """What the broker must run alone: under k_serve the J = 65 .. 67 reads, the 2048-base reads and the private tables -- no
    thin-body read of the set misses its cap there, and no `under` read counts; in the lanes form (thin bodies only) the `under`
    reads do, and the 2048-base reads do not."""
    serve = lanes = 0
    for b, (ee, _, _, rows) in zip(batches, results):
        hs, hl = SC.handed_back(b.pred, rows, np.isnan(ee), "serve"), SC.handed_back(b.pred, rows, np.isnan(ee), "lanes")
        body = b.pred.body()
        assert (hs == ((b.lens == 2048) | ((body == "reg") & (rows > 64)))).all()
        assert (rows[hs & (body == "reg")] <= 67).all()
        under = (body == "reg") & ~b.pred.amb & (b.pred.cap_hi < rows)
        assert (hl == under).all()
        serve, lanes = serve + int(hs.sum()), lanes + int(hl.sum())
    assert SC.solo_expected(oracle, batches, "serve") == serve + len(SC.PRIV)
    assert SC.solo_expected(oracle, batches, "lanes") == lanes + len(SC.PRIV)
    assert serve >= 4 and lanes >= 8 + 3
    seqs = SC.sequences(oracle, batches)
    want = SC.expected(oracle, batches)
    assert set(seqs) == {"long_short", "sthin_reg_sthin", "alphas"} and all(k in want for s in seqs.values() for k in s)
    ln = lambda k: int(batches[k[0]].lens[k[1]])
    assert [ln(k) for k in seqs["long_short"][:4]] == [2047, 1, 2047, 2] and 1024 in [ln(k) for k in seqs["long_short"]]
    bodies = [batches[k[0]].pred.body()[k[1]] for k in seqs["sthin_reg_sthin"]]
    assert bodies[:5] == ["sthin", "reg", "sthin", "reg", "sthin"]
    al = [batches[k[0]].alpha for k in seqs["alphas"]]
    assert set(al) == set(SC.ALPHAS) and all(al[i] != al[i + 1] for i in range(len(al) - 1))
    assert sum(len(s) for s in seqs.values()) < 100
