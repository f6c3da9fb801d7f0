"""The sorted pipeline's front end on the GPU -- k_prepass (RAGGED x LONG x LISTED), k_classify_linear<., DECODE>, k_scan, k_tables --
against tests/helpers/front_end_model.py.  The final ee / pass are insensitive to these kernels by design (a read whose budget
is wrong is repaired by the overflow pass), so every run here also pins what they alone decide:

  (a) ee, ns, pass equal the oracle bit for bit, guards intact
  (b) mpb_last_read_budgets equals the float64 model's cap on every SURE read (budget the same at both ends of the band
      0.01 + 1e-5 |x|); at most 5 % of a batch is unsure, and an unsure read gets one of its two bracketing caps
  (c) mpb_last_class_histogram is bincount(budgets) over the 32 caps, exactly; the reads it misses are those of budget 0
  (d) n_overflow lies in [A, A + U]: A = sure tile reads whose oracle rows exceed their budget, U = unsure and wide reads
  (e) a second run reports the same budgets

at the shapes where the code changes path: n around 16 / 64 / 256 / 1024, 256 and 257 blocks (k_scan), strides on both sides of
960 (k_prepass' LONG instance) and of its 960-byte panels, 16-read groups of mixed lengths, rows of ambiguity markers, the
strides at which k_classify_linear's tile geometry changes, and lists of 1 .. 1025 reads handed back by a forced narrow pass.
Every run prints its figures (unsure share, sure reads that disagree) before it asserts.

(b) is why k_prepass and k_classify_linear sum a lane's bytes a second time when they meet an 'n': its marker, 65536 in the float
that also carries sum p (1 - p), leaves that sum steps of 2^-7, more than a good base adds, and the budget went with it.
The LISTED runs cannot read budgets (mpb_last_read_budgets describes whole batches only): there the list is pinned by results,
n_fallback and the n_overflow bracket over the handed-back reads."""
import numpy as np
import pytest

from helpers import class_cells as CC
from helpers import front_end_model as FM
from helpers.device_runs import Resident, classified_pair, same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from moira_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def want(oracle):
    """batch -> (ee, ns, pass, rows) of the oracle: computed once per batch, shared by the resident and the classified tests."""
    cache = {}

    def get(b):
        if b.name.startswith("scan%d_" % FM.SCAN_N[0]):               # the first rows of the larger scan batch
            return tuple(v[:b.n] for v in get(FM.scan_batch(FM.SCAN_N[1], b.fixed_len is None)))
        if b.name not in cache:
            cache[b.name] = oracle.filter_batch(b.q, lens=b.lens, alpha=b.alpha, threads=16)
        return cache[b.name]
    return get


_MODELS = {}


def model_of(b, under=False):
    if (b.name, under) not in _MODELS:
        _MODELS[b.name, under] = FM.Model(b.q, b.lens, b.alpha, under)
    return _MODELS[b.name, under]


def check_front_end(b, under, got, budgets, hist, n_overflow, exp, label):
    """Assertions (a) - (d) of one run; got = (ee, ns, pass)."""
    ee, ns, ps = got
    assert same(ee, exp[0]), (label, "ee", int((ee != exp[0]).sum()))                                           # (a)
    assert np.array_equal(ns, exp[1]), (label, "ns", np.flatnonzero(ns != exp[1])[:8])
    assert np.array_equal(np.asarray(ps).astype(bool), exp[2].astype(bool)), (label, "pass")
    m = model_of(b, under)                                                                                      # (b)
    wrong = np.flatnonzero(m.sure & (budgets != m.budget))
    print("[front end] %-28s n %7d  alpha %-6g  unsure %.4f  sure reads that disagree %d  n_overflow %d"
          % ("%s%s" % (label, " under" if under else ""), b.n, b.alpha, m.unsure_share, len(wrong), n_overflow))
    assert m.unsure_share <= FM.UNSURE_MAX, (label, m.unsure_share)
    assert len(wrong) == 0, (label, len(wrong), [(int(i), int(b.lens[i]), float(m.x[i]), int(m.budget[i]), int(budgets[i]))
                                                 for i in wrong[:6]])
    loose = ~m.sure
    assert ((budgets[loose] == m.lo[loose]) | (budgets[loose] == m.hi[loose])).all(), label
    assert sorted(hist) == [int(c) for c in CC.CAPS], label                                                     # (c)
    counted = np.array([hist[int(c)] for c in CC.CAPS])
    assert np.array_equal(counted, np.bincount(np.searchsorted(CC.CAPS, budgets[budgets > 0]), minlength=len(CC.CAPS))), label
    assert np.isin(budgets, np.r_[0, CC.CAPS]).all() and counted.sum() == b.n - int((budgets == 0).sum()), label
    lo, hi = FM.overflow_bracket(m, exp[3])                                                                     # (d)
    assert lo <= n_overflow <= hi, (label, lo, n_overflow, hi)
    return m


def run_resident(eng, b, exp):
    """mpb_filter_device with MPB_FLAG_NO_NARROW, plain (twice: (e)) and with MPB_FLAG_TEST_UNDERPREDICT."""
    res = Resident(eng, b.q, b.lens if b.fixed_len is None else None)
    try:
        first = None
        for under in (False, False, True):
            ee, ns, ps, c, path, intact = res.run(fixed_len=b.fixed_len, alpha=b.alpha, no_narrow=True, test_underpredict=under)
            budgets = eng.read_budgets(b.n)
            assert intact and path["narrow_rows"] == 0 and (c.n_reads, c.n_pass) == (b.n, int(exp[2].sum())), b.name
            if first is None:
                first = budgets
                check_front_end(b, under, (ee, ns, ps), budgets, eng.class_histogram(), c.n_overflow, exp, b.name)
            elif not under:
                assert np.array_equal(budgets, first), (b.name, "second run")                                   # (e)
            else:
                check_front_end(b, under, (ee, ns, ps), budgets, eng.class_histogram(), c.n_overflow, exp, b.name)
    finally:
        res.free()


def run_classified(eng, b, exp):
    """The batch as text through mpb_decode_classify_device + mpb_filter_device_classified (k_classify_linear<., DECODE>)."""
    zeroed = np.where(np.arange(b.stride)[None, :] < b.lens[:, None], b.q, 0).astype(np.uint8)
    for under in (False, True):
        ee, ns, ps, c, budgets, hist, packed, intact = classified_pair(eng, b.q, b.lens, fixed_len=b.fixed_len, front_end=True,
                                                                       alpha=b.alpha, test_underpredict=under)
        assert intact and np.array_equal(packed, zeroed), (b.name, "guards, packed matrix")
        assert (c.n_reads, c.n_pass) == (b.n, int(exp[2].sum())), b.name
        check_front_end(b, under, (ee, ns, ps), budgets, hist, c.n_overflow, exp, b.name + " text")


LAYOUTS = ("ragged",) + tuple("fixed-%d" % c for c in FM.FIXED_CUTS)


def _sweep(stride, layout):
    return FM.sweep_batch(stride, None if layout == "ragged" else int(layout.split("-")[1]))


@pytest.mark.parametrize("ragged", [False, True], ids=["fixed40", "ragged"])
def test_n_sweep_resident_and_classified(eng, want, ragged):
    """1 .. 2049 reads at stride 48: a lane group, a wave, a round of four waves and a block of 1024, one read short and one over."""
    for n in FM.N_SWEEP:
        b = FM.n_sweep_batch(n, ragged)
        run_resident(eng, b, want(b))
        run_classified(eng, b, want(b))


@pytest.mark.parametrize("n", FM.SCAN_N)
@pytest.mark.parametrize("ragged", [False, True], ids=["fixed32", "ragged"])
def test_scan_boundary(eng, want, n, ragged):
    """256 and 257 blocks: k_scan's threads go from one block histogram each to two.  A ragged batch scans 16 length bins per class."""
    b = FM.scan_batch(n, ragged)
    run_resident(eng, b, want(b))
    run_classified(eng, b, want(b))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("stride", sorted(FM.SWEEP))
def test_stride_sweep_resident(eng, want, stride, layout):
    """k_prepass at 1,100 reads: 16-read groups that hold an empty row, a full one and lengths on both sides of a 16-byte chunk;
    fixed lengths stride, stride - 1, stride - 15, stride - 16; strides on both sides of 960 (LONG) and of two panels."""
    b = _sweep(stride, layout)
    run_resident(eng, b, want(b))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("stride", sorted(FM.SWEEP))
def test_stride_sweep_classified(eng, want, stride, layout):
    b = _sweep(stride, layout)
    run_classified(eng, b, want(b))


@pytest.mark.parametrize("stride", FM.MARKER_STRIDES)
def test_marker_peel(eng, want, stride):
    """Rows of 'N' / 'n' (128 / 65536 in the float sum the counts are peeled off, panel by panel): ns exact, and the budget
    by the scored + 1 clamp -- a row without a scored base has one DP row (cap 2), one with a single scored base at most two."""
    b = FM.marker_batch(stride)
    exp = want(b)
    for i, kind, L in b.kinds:
        row = b.q[i, :L]
        assert exp[1][i] == int(((row == 0) | (row == 255)).sum()), (kind, L)
    run_resident(eng, b, exp)
    run_classified(eng, b, exp)
    m = model_of(b)
    for i, kind, L in b.kinds:
        if not kind.startswith("scored_last_chunk"):
            assert m.sure[i] and m.budget[i] == 2, (kind, L)


@pytest.mark.parametrize("ragged", [True, False], ids=["ragged", "fixed"])
@pytest.mark.parametrize("stride", sorted(FM.LINEAR_GEOMETRY))
def test_linear_geometry_classified(eng, want, stride, ragged):
    """k_classify_linear where tile_rows = 1280 / cpr, the lanes per row and c / cpr by magic multiply change: cpr 2, 3, 5,
    79 / 80 / 81, 640 / 641, 1024.  Below stride 10240 a block walks whole tiles and a partial one; from there on 40 reads, one
    of them wide."""
    b = FM.linear_batch(stride, ragged)
    assert FM.linear_geometry(stride) == FM.LINEAR_GEOMETRY[stride]
    run_classified(eng, b, want(b))
    run_resident(eng, b, want(b))


@pytest.mark.parametrize("ragged", [False, True], ids=["fixed", "ragged"])
@pytest.mark.parametrize("m", FM.LISTED_M)
def test_listed_prepass_over_the_reads_a_narrow_pass_hands_back(eng, oracle, m, ragged):
    """k_prepass<., ., LISTED>: a forced two-row narrow pass hands exactly m planted reads back, and the sorted pipeline runs over
    that list where the reads lie.  mpb_filter_counts.n_overflow of such a call is the list's own (fetch_counts copies the counter
    k_tables zeroed for the sub-batch; mpb_resident.cpp), so it is bracketed by the model over the handed-back reads alone: a
    prepass that indexed by position instead of by read would class other reads' bytes."""
    b, at, exp = FM.listed_batch(oracle, m, ragged)
    live = np.arange(b.stride)[None, :] < b.lens[:, None]
    back = (exp[3] > 2) | (live & (b.q == 255)).any(1)
    assert np.array_equal(np.flatnonzero(back), at) and 2 * m <= b.n
    res = Resident(eng, b.q, b.lens if ragged else None)
    try:
        ee, ns, ps, c, path, intact = res.run(fixed_len=b.fixed_len, alpha=b.alpha, narrow_rows=2)
    finally:
        res.free()
    assert same(ee, exp[0]) and np.array_equal(ns, exp[1]) and np.array_equal(ps.astype(bool), exp[2].astype(bool)) and intact
    assert path["narrow_rows"] == 2 and path["n_fallback"] == m and c.n_pass == int(exp[2].sum())
    model = FM.Model(b.q, b.lens, b.alpha)
    lo, hi = FM.overflow_bracket(model, exp[3], among=back)
    print("[front end] %-28s handed back %5d  unsure among them %d  n_overflow %d in [%d, %d]"
          % (b.name, m, int((back & ~model.sure).sum()), c.n_overflow, lo, hi))
    assert model.unsure_share <= FM.UNSURE_MAX and int((back & ~model.sure).sum()) <= FM.UNSURE_MAX * m, b.name
    assert lo <= c.n_overflow <= hi, (b.name, lo, c.n_overflow, hi)
