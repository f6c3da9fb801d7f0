"""Directed inputs for every DP class body: each batch of tests/helpers/class_cells.py through every entry of the library, bit
for bit against the oracle, and a LEDGER -- built from the budgets the library itself reports (mpb_last_read_budgets) and the
oracle's rows -- that says which (class, crossing row) cells really ran: lane boundaries of the two-phase CDF walk, the first and
last row of every class, the early lanes of the wide classes (overflow pass), the tile / wide boundary, k_wide's wave
boundaries, the ten one-read-per-wave bodies.  An empty cell fails the test by name.  Then the result arrays and the matrix as
SUB-VIEWS of larger allocations (k_narrow_rs' unaligned store path), with guard elements around them."""
import numpy as np
import pytest

from helpers import class_cells as CC
from helpers.device_runs import Resident, classified_pair, matrix_offset_is_refused, same, seq_and_quals

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from moira_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def batches(oracle):
    return CC.generate(oracle)


@pytest.fixture(scope="module")
def want(oracle, batches):
    """{batch name: (ee, ns, pass, rows)}: the oracle once per batch (default flags: --ambigs treat_as_errors, uncert 0.01)."""
    return {b.name: oracle.filter_batch(b.q, lens=b.lens, alpha=b.alpha, threads=8) for b in batches}


def check(got, exp, label):
    ee, ns, ps = got[:3]
    assert same(ee, exp[0]), (label, int((ee != exp[0]).sum()))
    assert np.array_equal(ns, exp[1]) and np.array_equal(np.asarray(ps).astype(bool), exp[2].astype(bool)), label


@pytest.fixture(scope="module")
def device_runs(eng, batches, want):
    """Every batch through mpb_filter_device (sorted pipeline), plain and with MPB_FLAG_TEST_UNDERPREDICT, with the budgets and
    counters of each run: {name: {under: (ee, ns, pass, counts, budgets, caps of the class histogram)}}."""
    out = {}
    for b in batches:
        res = Resident(eng, b.q, b.lens)
        out[b.name] = {}
        for under in (False, True):
            ee, ns, ps, c, path, intact = res.run(fixed_len=b.fixed_len, alpha=b.alpha, no_narrow=True, test_underpredict=under)
            assert intact and path["narrow_rows"] == 0
            out[b.name][under] = (ee, ns, ps, c, eng.read_budgets(b.n), sorted(eng.class_histogram()))
        res.free()
    return out


def test_filter_device_is_the_oracle_with_and_without_underpredict(batches, want, device_runs):
    for b in batches:
        for under in (False, True):
            got = device_runs[b.name][under]
            check(got, want[b.name], (b.name, under))
            assert (got[3].n_reads, got[3].n_pass) == (b.n, int(want[b.name][2].sum()))


def test_class_caps_are_the_histograms(batches, device_runs):
    """mpb_last_class_histogram lists the 32 caps of MPB_CLASSES; every budget is one of them (0: a wide read)."""
    for b in batches:
        caps, budgets = device_runs[b.name][False][5], device_runs[b.name][False][4]
        assert caps == [int(c) for c in CC.CAPS], b.name
        assert np.isin(budgets, np.r_[0, CC.CAPS]).all()
        if b.stride < 1024:
            assert (budgets > 0).all()


def test_no_main_pass_cell_is_empty(batches, want, device_runs):
    """Main pass, from the real budgets: every tile class at js = prev, js = cap - 1 and both sides of each lane boundary in
    between (170 cells); the tile / wide boundary and k_wide's wave boundaries; the ten thin bodies."""
    filled = set()
    for b in batches:
        if b.kind == "ovf":
            continue
        rows, budgets = want[b.name][3], device_runs[b.name][False][4]
        filled |= CC.ledger_main(rows, budgets) | CC.ledger_wide(rows, budgets)
        if b.stride <= 2048:                                  # these also go through the one-read-per-wave entries below
            filled |= CC.ledger_thin(rows, budgets)
    for group, req in (("main", CC.main_cells()), ("wide", CC.WIDE_CELLS), ("thin", CC.thin_cells())):
        miss = CC.missing(req, filled)
        assert not miss, "%s cells no read reached (class, crossing row): %s" % (group, miss)
    assert len(CC.main_cells()) == 170


def test_no_overflow_pass_cell_is_empty(oracle, batches, want, device_runs):
    """MPB_FLAG_TEST_UNDERPREDICT, from the real (halved) budgets: a read whose budget misses is re-run by the class that covers
    max_len + 1 rows -- fixed_len + 1 here, and the widest tile class for the ragged stride-960 batches -- so it crosses in that
    class's EARLY lanes: lane 0, both sides of the lane 0 / 1 boundary and of the one at G / 2, the first row of the last lane."""
    filled = set()
    for b in batches:
        rows, budgets = want[b.name][3], device_runs[b.name][True][4]
        if b.kind == "ovf":
            filled |= CC.ledger_overflow(rows, budgets, b.final_cap)
        elif b.stride == 960:
            filled |= CC.ledger_overflow(rows, budgets, 1024)
    miss = CC.missing(CC.overflow_cells(oracle), filled)
    assert not miss, "overflow cells no read reached (class, crossing row): %s" % miss


def test_n_overflow_counts_the_reads_whose_budget_missed(batches, want, device_runs):
    """mpb_filter_counts.n_overflow = reads whose CDF did not cross inside their row budget: J > budget for a read of a tile
    class.  A wide read's budget (its predicted rows) is reported by no entry, so a batch that holds wide reads can only bound
    the count here; test_gpu_no_crossing.py pins the wide part where every budget is known (1 - alpha == 1)."""
    some = 0
    for b in batches:
        rows = want[b.name][3]
        for under in (False, True):
            c, budgets = device_runs[b.name][under][3], device_runs[b.name][under][4]
            tile = int(((budgets > 0) & (rows > budgets)).sum())
            wide = int((budgets == 0).sum())
            assert tile <= c.n_overflow <= tile + wide, (b.name, under)
            if wide == 0:
                assert c.n_overflow == tile, (b.name, under)        # no wide read: the count is exact
            some += c.n_overflow
    assert some > 500


@pytest.mark.parametrize("under", [False, True])
def test_host_entry_sorted_pipeline(eng, batches, want, device_runs, under):
    """Engine.filter with batched_only and no_narrow, then read_budgets: the host entry classes a read as the device entry does."""
    for b in batches:
        r = eng.filter(b.q, alpha=b.alpha, batched_only=True, no_narrow=True, test_underpredict=under, **b.len_kw())
        check((r.ee, r.ns, r.passed), want[b.name], b.name)
        assert r.n_pass == int(want[b.name][2].sum()) and r.n_overflow == device_runs[b.name][under][3].n_overflow
        assert np.array_equal(eng.read_budgets(b.n), device_runs[b.name][under][4]), b.name


def small_path_launches(eng, q, **kw):
    """Engine.filter with kernel timing on -> (result, launches of the classification pass): 0 = the one-read-per-wave kernel
    finished every read; the sorted pipeline, which a missed budget or a wide read sends the whole batch to, classifies first."""
    eng.timing(True)
    eng.timing_reset()
    try:
        r = eng.filter(q, **kw)
        return r, eng.kernel_times()["prepass"][1]
    finally:
        eng.timing(False)


@pytest.mark.parametrize("under", [False, True])
def test_small_path(eng, batches, want, device_runs, under):
    """Batches of at most 4096 reads without MPB_FLAG_BATCHED_ONLY: one read per wave, the thin bodies.  One wide read, or one
    read whose budget misses, sends the WHOLE batch down the pipeline, so besides each batch as it is, the reads whose budget
    holds (tile class, J <= budget: the reads the thin ledger counts) go in as a batch of their own -- and that one must be
    finished by the one-read-per-wave kernel alone."""
    for b in batches:
        assert b.n <= 4096
        r = eng.filter(b.q, alpha=b.alpha, test_underpredict=under, **b.len_kw())
        check((r.ee, r.ns, r.passed), want[b.name], b.name)
        assert r.n_pass == int(want[b.name][2].sum())
        budgets = device_runs[b.name][under][4]
        keep = np.nonzero((budgets > 0) & (want[b.name][3] <= budgets))[0]
        if len(keep) == 0 or b.stride > 2048:
            continue
        kw = dict(fixed_len=b.fixed_len) if b.fixed_len is not None else dict(lens=b.lens[keep])
        r, classified = small_path_launches(eng, np.ascontiguousarray(b.q[keep]), alpha=b.alpha, test_underpredict=under, **kw)
        check((r.ee, r.ns, r.passed), [x[keep] for x in want[b.name]], (b.name, "sub-batch"))
        assert classified == 0, (b.name, under)


def test_classified_at_source_pair(eng, batches, want):
    for b in batches:
        ee, ns, ps, c = classified_pair(eng, b.q, b.lens, fixed_len=b.fixed_len, alpha=b.alpha)
        check((ee, ns, ps), want[b.name], b.name)
        assert c.n_pass == int(want[b.name][2].sum())


def test_per_read_entry_on_the_thin_and_wide_boundary_reads(eng, oracle, batches, want, device_runs):
    """bernoulli.calculate_errors_PB's twin, read by read (the resident one-read kernel, k_serve): up to two reads per thin cell
    and per wide cell of the ledger, and every read of the stride-4096 batches.  The thin ledger names the body k_small runs
    (test_small_path).  Under k_serve a read of at most 1024 bases and at most 64 predicted rows runs the register-resident body
    instead, so of the reads picked here only those of more than 1024 bases or of caps 128 .. 1024 run the thin body the ledger
    names, a read of more than 2047 bases takes the host path, and the wide cells are handed back by the kernel and answered by
    the host.  The register body's own cells, and the thin bodies of cap <= 64 as k_serve runs them (reads of 1025 .. 2047
    bases), are tests/test_gpu_serve_edges.py's."""
    todo = []
    seen = {}
    for b in batches:
        if b.kind == "ovf":
            continue
        rows, budgets = want[b.name][3], device_runs[b.name][False][4]
        for i in range(b.n):
            cells = CC.ledger_thin(rows[i:i + 1], budgets[i:i + 1]) | CC.ledger_wide(rows[i:i + 1], budgets[i:i + 1])
            cells &= set(CC.thin_cells()) | set(CC.WIDE_CELLS)
            if b.stride == 4096 or any(seen.get((c, b.alpha), 0) < 1 for c in cells):
                for c in cells:
                    seen[(c, b.alpha)] = seen.get((c, b.alpha), 0) + 1
                todo.append((b, i))
    assert 60 <= len(todo) <= 600
    for b, i in todo:
        seq, quals = seq_and_quals(b.q[i], int(b.lens[i]))
        got = eng.calculate_errors_PB(seq, quals, b.alpha)
        exp = oracle.ee_rowwise(seq, quals, b.alpha)
        assert got == exp[:2], (b.name, i, exp[2])


# ---- sub-views ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", CC.NARROW_LAYOUTS)
def test_sub_views_of_larger_buffers(eng, oracle, layout):
    """The ABI promises 16-byte alignment for the matrix and none for the result arrays: the matrix 16, 32, 64 and 80 bytes into
    its allocation, d_ee / d_ns / d_pass one element into theirs (k_narrow_rs then cannot store pairs).  Results equal the
    aligned run's and the oracle's, through the sorted pipeline and every forced narrow form; the elements before and after
    each result array are untouched; the narrow pass hands back exactly the reads the oracle's rows say it cannot finish."""
    q, lens, fixed = CC.narrow_batch(oracle, layout)
    exp = oracle.filter_batch(q, lens=lens, threads=8)
    rows = exp[3]
    live = np.arange(q.shape[1])[None, :] < lens[:, None]
    has_n = (live & (q == 255)).any(1)
    filled = set()
    aligned = Resident(eng, q, None if fixed else lens)
    base = {}
    for R in (0, 2, 3, 4):
        kw = dict(narrow_rows=R) if R else dict(no_narrow=True)
        got = aligned.run(fixed_len=fixed, **kw)
        check(got, exp, (layout, R))
        assert got[5] and got[4]["narrow_rows"] == R
        if R:
            assert got[4]["n_fallback"] == int(((rows > R) | has_n).sum()), (layout, R)
            filled |= CC.ledger_narrow(layout, R, q, lens, rows)
        base[R] = got
    assert matrix_offset_is_refused(eng, aligned, 8) == -1           # MPB_E_INVALID
    assert b"16-byte aligned" in eng.lib.mpb_last_error()
    aligned.free()
    assert CC.missing([c for c in CC.narrow_cells() if c[1] == layout], filled) == []
    for q_off in (16, 32, 64, 80):
        view = Resident(eng, q, None if fixed else lens, q_offset=q_off, res_offset=1)
        assert view.ptrs()[1] % 16 == 8 and view.ptrs()[2] % 8 == 4 and view.ptrs()[3] % 2 == 1
        for R in (0, 2, 3, 4):
            kw = dict(narrow_rows=R) if R else dict(no_narrow=True)
            ee, ns, ps, c, path, intact = view.run(fixed_len=fixed, **kw)
            assert intact, (layout, q_off, R)
            assert same(ee, base[R][0]) and np.array_equal(ns, base[R][1]) and np.array_equal(ps, base[R][2]), (layout, q_off, R)
            assert path["narrow_rows"] == R and path["n_fallback"] == base[R][4]["n_fallback"]
            assert c.n_pass == base[R][3].n_pass == int(exp[2].sum())
        view.free()
