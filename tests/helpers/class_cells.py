"""Directed inputs for the DP class bodies: which (class, crossing row) cells a batch must reach, a generator that reaches
them, and the ledger that says which were reached.  Plain Python and numpy; no GPU.

A read's DP runs in the class body its PREDICTED row count selects (moira_amd/csrc/mpb_internal.h: MPB_CLASSES), and its result
is read off the row `js` where its CDF first exceeds 1 - alpha (J = js + 1 rows are needed; the oracle reports J as `rows`).
The places of a body that have code of their own are rows, so a test aims at (class, js) cells:

  main      a read of tile class `cap` (previous class's cap `prev`, or 0) crosses in rows prev .. cap - 1 when the predictor
            does not under-predict; required: js = prev, js = cap - 1 and both sides of every lane boundary g * R in between
  overflow  with MPB_FLAG_TEST_UNDERPREDICT a read whose halved budget misses is re-run by ONE class, the smallest whose
            cap covers max_len + 1 rows (mpb_launch_overflow; max_len = fixed_len, or the row stride of a ragged batch; the
            wide kernel when max_len + 1 > 1024), so there a read crosses in the EARLY lanes of a wide class; required per
            class with G > 1: a row of lane 0, both sides of the lane 0 / 1 boundary, both sides of the boundary at
            g = G / 2, the first row of the last lane -- where a read can reach it (see overflow_unreachable)
  wide      the tile / wide boundary (budget 1024 with J = 1024; a wide read with J <= 1024) and k_wide's wave boundaries
            (js = 1023, 1024, 2047, 2048); every wave boundary of all four k_wide instances, both passes and the list loop:
            helpers/wide_cells.py
  thin     the ten one-read-per-wave bodies (MPB_THIN_CLASSES: cap = the next power of two >= the predicted rows):
            first reachable row (cap / 2; 0 for cap 2), last row, and one lane boundary (g = 3 G / 4) where R > 1.  These are the
            bodies of k_small (a launch per batch of at most 4096 reads, or per call with MPB_SERVE=0).  The resident kernel
            k_serve, which answers a per-read call, runs them only for a read of more than 1024 bases or more than 64 predicted
            rows; any other read runs its register-resident body, whose cells are helpers/serve_cells.py's
  modes     MPB_FLAG_FAST_FMA and MPB_FLAG_ODDS compile every class body once more, so the main cells are required again per
            mode, by the crossing row of the mode's CPU model (generate(mode=...), ledger_mode); ODDS keeps a read only while
            p0 >= 2^-900, which puts the far rows of class 1024 out of every read's reach (odds_unreachable)
  narrow    the natural-order narrow forms (2, 3, 4 rows): crossing on row 0, on row R - 1, on row R (handed back), a read of
            only 'N', a read with an 'n', and a zero-length read in ragged batches

The predictor model below only STEERS the generator (which candidate reads to keep).  What a test asserts comes from the
oracle's rows and, on the GPU, from the budgets the library itself reports.
"""
import math
import re
from concurrent.futures import ThreadPoolExecutor

import numpy as np

# (cap, G, R): G lanes cooperate on a read, R rows each.  Restated from MPB_CLASSES / MPB_THIN_CLASSES; test_class_cells.py
# checks this text against the header's.
TILE_CLASSES = tuple((r * g, g, r) for r, g in (
    (2, 1), (3, 1), (4, 1), (5, 1), (6, 1), (7, 1), (8, 1), (9, 1), (10, 1), (12, 1), (14, 1), (16, 1),
    (10, 2), (12, 2), (14, 2), (16, 2), (10, 4), (12, 4), (14, 4), (16, 4),
    (9, 8), (10, 8), (11, 8), (12, 8), (14, 8), (16, 8), (10, 16), (12, 16), (16, 16), (12, 32), (16, 32), (16, 64)))
THIN_CLASSES = tuple((r * g, g, r) for r, g in (
    (1, 2), (1, 4), (1, 8), (1, 16), (1, 32), (1, 64), (2, 64), (4, 64), (8, 64), (16, 64)))
TILE_MAX_ROWS = 1024
CAPS = np.array([c[0] for c in TILE_CLASSES], np.int32)
ALPHAS = (0.005, 0.05, 1e-6)
MODES = ("fma", "odds")                   # MPB_FLAG_FAST_FMA, MPB_FLAG_ODDS: each compiles every class body once more
MODE_ALPHAS = (0.005, 0.05, 1e-5)         # both modes refuse alpha < 1e-5


def parse_header_classes(text):
    """{macro: [(cap, G, R)]} of the X(id, R, G) lists in mpb_internal.h, in id order."""
    out = {}
    for name in ("MPB_CLASSES", "MPB_THIN_CLASSES"):
        m = re.search(r"#define\s+%s\(X\)((?:[^\n]*\\\n)*[^\n]*)" % name, text)
        ent = [tuple(int(v) for v in e) for e in re.findall(r"X\(\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*\)", m.group(1))]
        assert [e[0] for e in ent] == list(range(len(ent))), name
        out[name] = [(r * g, g, r) for _, r, g in ent]
    return out


def prev_cap(cap):
    k = int(np.searchsorted(CAPS, cap))
    assert CAPS[k] == cap
    return int(CAPS[k - 1]) if k else 0


def class_of(cap):
    return TILE_CLASSES[int(np.searchsorted(CAPS, cap))]


def cap_of_rows(rows):
    """Budget of a predicted row count: the smallest tile cap >= rows, 0 for a wide read (what mpb_last_read_budgets reports)."""
    rows = np.asarray(rows)
    k = np.searchsorted(CAPS, np.minimum(rows, TILE_MAX_ROWS))
    return np.where(rows > TILE_MAX_ROWS, 0, CAPS[np.minimum(k, len(CAPS) - 1)]).astype(np.int32)


def thin_cap_of_budget(budget):
    """The one-read-per-wave body of a read whose tile budget is `budget`: cap 2^(id + 1), id = ceil(log2(rows)) - 1.  Every
    tile class lies inside one power-of-two interval, so the tile budget names the thin body (0 = wide: the host re-runs it)."""
    b = np.asarray(budget).astype(np.int64)
    return np.where(b <= 0, 0, np.maximum(2, 1 << np.ceil(np.log2(np.maximum(b, 1))).astype(np.int64))).astype(np.int32)


# ---- the predictor ---------------------------------------------------------------------------------------------------

def inv_norm_cdf(p):
    """Acklam's rational approximation, as make_dev_params evaluates it."""
    a = (-3.969683028665376e+01, 2.209460984245205e+02, -2.759285104469687e+02, 1.383577518672690e+02,
         -3.066479806614716e+01, 2.506628277459239e+00)
    b = (-5.447609879822406e+01, 1.615858368580409e+02, -1.556989798598866e+02, 6.680131188771972e+01, -1.328068155288572e+01)
    c = (-7.784894002430293e-03, -3.223964580411365e-01, -2.400758277161838e+00, -2.549732539343734e+00,
         4.374664141464968e+00, 2.938163982698783e+00)
    d = (7.784695709041462e-03, 3.224671290700398e-01, 2.445134137142996e+00, 3.754408661907416e+00)
    tail = lambda q: (((((c[0] * q + c[1]) * q + c[2]) * q + c[3]) * q + c[4]) * q + c[5]) / \
                     ((((d[0] * q + d[1]) * q + d[2]) * q + d[3]) * q + 1)
    if p < 0.02425:
        return tail(math.sqrt(-2 * math.log(p)))
    if p > 1 - 0.02425:
        return -tail(math.sqrt(-2 * math.log(1 - p)))
    q = p - 0.5
    r = q * q
    return (((((a[0] * r + a[1]) * r + a[2]) * r + a[3]) * r + a[4]) * r + a[5]) * q / \
           (((((b[0] * r + b[1]) * r + b[2]) * r + b[3]) * r + b[4]) * r + 1)


def _stat_tables():
    f = np.float32
    code = np.arange(256, dtype=np.float32)
    p = np.exp2(f(-0.33219281) * code).astype(f)
    p[0] = p[255] = 0
    v = (p * (f(1) - p)).astype(f)
    v[0] = v[255] = 0
    return p, v, (p * v).astype(f)


def read_stats(q, lens):
    """(mu, var, k3, scored) of every read of a packed matrix, float32: sums of p, p(1-p), p(1-p)(1-2p) over the scored bases."""
    f = np.float32
    tp, tv, ts = _stat_tables()
    q = np.asarray(q)
    lens = np.asarray(lens)
    live = np.arange(q.shape[1])[None, :] < lens[:, None]
    code = np.where(live, q, np.uint8(0))
    mu = tp[code].sum(1, dtype=f)
    var = tv[code].sum(1, dtype=f)
    k3 = (var - f(2) * ts[code].sum(1, dtype=f)).astype(f)
    scored = (live & (q != 0) & (q != 255)).sum(1)
    return mu, var, k3, scored


def rows_from_stats(stats, alpha, underpredict=False):
    f = np.float32
    mu, var, k3, scored = stats
    z = inv_norm_cdf(1 - alpha)
    z32, zq = f(z), f((z * z - 1) / 6)
    v = np.maximum(var, f(1e-12))
    x = (mu + z32 * np.sqrt(v) + (k3 / v) * zq).astype(f)
    rows = np.floor(np.minimum(x, f(1e9)) + f(0.5)).astype(np.int64) + 1
    if underpredict:
        rows = rows // 2
    return np.maximum(np.minimum(rows, scored + 1), 1).astype(np.int32)


def predicted_rows(q, lens, alpha, underpredict=False):
    """float32 model of class_read()'s row prediction for every read of a packed matrix: mu, var, k3, z = Phi^-1(1 - alpha),
    zq = (z^2 - 1) / 6, x = mu + z sqrt(var) + (k3 / var) zq, rows = floor(x + 0.5) + 1, halved under
    MPB_FLAG_TEST_UNDERPREDICT, clamped to 1 .. scored + 1.  The kernels sum in another order and take p from the hardware's
    exp2, so a read on the edge of a class may land next door: steering only."""
    return rows_from_stats(read_stats(q, lens), alpha, underpredict)


# ---- required cells --------------------------------------------------------------------------------------------------

def main_cells():
    """[("main", cap, js)]: 170 cells."""
    out = []
    for cap, G, R in TILE_CLASSES:
        prev = prev_cap(cap)
        rows = {prev, cap - 1}
        for g in range(1, G):
            if prev <= g * R - 1 and g * R <= cap - 1:
                rows |= {g * R - 1, g * R}
        out += [("main", cap, js) for js in sorted(rows)]
    return out


def overflow_cells_all():
    """[("ovf", cap, what)] for every class with G > 1, reachable or not; what = "lane0" (any js < R) or a row."""
    out = []
    for cap, G, R in TILE_CLASSES:
        if G > 1:
            out.append(("ovf", cap, "lane0"))
            out += [("ovf", cap, js) for js in sorted({R - 1, R, (G // 2) * R - 1, (G // 2) * R, (G - 1) * R})]
    return out


OVF_ALPHA_LADDER = (1e-6, 1e-9, 1e-12, 1e-15)      # below 1e-15, 1 - alpha is within a few ulp of 1 and such reads never cross
OVF_DEEP_ALPHA = 1e-12                             # the extra alpha of the batches whose last-lane cell needs more than min(ALPHAS)


def overflow_max_rows(oracle, cap, alphas=OVF_ALPHA_LADDER):
    """The most rows a read of the batch that selects class `cap` for its overflow pass can need and still have a result: that
    batch holds reads of at most cap - 1 bases (max_len + 1 <= cap), the worst base is Q1 (p = 0.794; a score of 0 is clamped
    to 1), and J grows with every p and with 1 / alpha -- so the oracle's J of cap - 1 bases of Q1, at the smallest alpha at
    which that read's CDF still crosses, bounds it."""
    L = cap - 1
    q = np.ones((1, 16 * ((L + 15) // 16)), np.uint8)
    best = 0
    for alpha in alphas:
        ee, _, _, rows = oracle.filter_batch(q, fixed_len=L, alpha=alpha)
        if not np.isnan(ee[0]):
            best = max(best, int(rows[0]))
    return best


def overflow_unreachable(oracle):
    """The overflow cells no input can reach: crossing row js needs J = js + 1 rows, more than overflow_max_rows allows."""
    lim = {cap: overflow_max_rows(oracle, cap) for cap, G, R in TILE_CLASSES if G > 1}
    return [c for c in overflow_cells_all() if c[2] != "lane0" and c[2] + 1 > lim[c[1]]]


def overflow_alphas(oracle, cap):
    """The alphas of class cap's overflow batches: ALPHAS, and OVF_DEEP_ALPHA where a required cell is out of reach at min(ALPHAS)."""
    lim = overflow_max_rows(oracle, cap, (min(ALPHAS),))
    need = max(c[2] + 1 for c in overflow_cells(oracle) if c[1] == cap and c[2] != "lane0")
    return ALPHAS + ((OVF_DEEP_ALPHA,) if need > lim else ())


def overflow_cells(oracle):
    bad = set(overflow_unreachable(oracle))
    return [c for c in overflow_cells_all() if c not in bad]


WIDE_CELLS = [("wide", "budget1024_J1024"), ("wide", "wide_J<=1024"), ("wide", 1023), ("wide", 1024), ("wide", 2047), ("wide", 2048)]


def thin_cells():
    out = []
    for cap, G, R in THIN_CLASSES:
        rows = {cap // 2 if cap > 2 else 0, cap - 1}
        if R > 1:
            g = 3 * G // 4
            rows |= {g * R - 1, g * R}
        out += [("thin", cap, js) for js in sorted(rows)]
    return out


NARROW_LAYOUTS = ("fixed320", "fixed304", "ragged640")


def narrow_cells():
    out = []
    for lay in NARROW_LAYOUTS:
        for R in (2, 3, 4):
            out += [("narrow", lay, R, w) for w in ("row0", "rowR-1", "rowR", "onlyN", "has_n")]
            if lay.startswith("ragged"):
                out.append(("narrow", lay, R, "len0"))
    return out


# ---- ledgers ---------------------------------------------------------------------------------------------------------

def ledger_main(rows, budgets, nan=None):
    """Cells of the main pass a batch fills: reads whose CDF crosses inside their budget (J <= budget), by (budget, js)."""
    rows, budgets = np.asarray(rows), np.asarray(budgets)
    ok = (budgets > 0) & (rows >= 1) & (rows <= budgets)
    if nan is not None:
        ok &= ~np.asarray(nan)
    return {("main", int(b), int(j) - 1) for b, j in zip(budgets[ok], rows[ok])}


def ledger_overflow(rows, budgets, final_cap, nan=None):
    """Cells of the overflow pass: reads whose (halved) budget misses (J > budget, tile reads), re-run in class final_cap."""
    rows, budgets = np.asarray(rows), np.asarray(budgets)
    R = class_of(final_cap)[2]
    ok = (budgets > 0) & (rows > budgets) & (rows <= final_cap)
    if nan is not None:
        ok &= ~np.asarray(nan)
    out = {("ovf", int(final_cap), int(j) - 1) for j in rows[ok]}
    if any(c[2] < R for c in out):
        out.add(("ovf", int(final_cap), "lane0"))
    return out


def ledger_wide(rows, budgets, nan=None):
    rows, budgets = np.asarray(rows), np.asarray(budgets)
    live = rows >= 1 if nan is None else (rows >= 1) & ~np.asarray(nan)
    out = set()
    if ((budgets == TILE_MAX_ROWS) & (rows == TILE_MAX_ROWS) & live).any():
        out.add(("wide", "budget1024_J1024"))
    wide = (budgets == 0) & live
    if (wide & (rows <= TILE_MAX_ROWS)).any():
        out.add(("wide", "wide_J<=1024"))
    for js in (1023, 1024, 2047, 2048):
        if (wide & (rows == js + 1)).any():
            out.add(("wide", js))
    return out


def ledger_thin(rows, budgets, nan=None):
    """Cells of the one-read-per-wave bodies: the body is named by the tile budget (thin_cap_of_budget)."""
    rows, budgets = np.asarray(rows), np.asarray(budgets)
    tc = thin_cap_of_budget(budgets)
    ok = (tc > 0) & (rows >= 1) & (rows <= np.maximum(budgets, 0))
    if nan is not None:
        ok &= ~np.asarray(nan)
    return {("thin", int(c), int(j) - 1) for c, j in zip(tc[ok], rows[ok])}


def ledger_mode(model, budgets):
    """Main-pass cells a batch fills under MPB_FLAG_FAST_FMA or MPB_FLAG_ODDS: reads the mode keeps (not handed to the exact
    pass) whose MODEL crosses inside their budget, by (budget, model rows - 1)."""
    return ledger_main(model.rows, budgets, nan=model.hand)


def ledger_thin_mode(model, budgets):
    """The same for the one-read-per-wave bodies (MPB_FLAG_FAST_FMA only: k_small has no ODDS form)."""
    return ledger_thin(model.rows, budgets, nan=model.hand)


def ledger_narrow(layout, R, q, lens, rows):
    """Cells of one narrow form on one batch, from the oracle's rows and the bytes alone."""
    q, lens, rows = np.asarray(q), np.asarray(lens), np.asarray(rows)
    live = np.arange(q.shape[1])[None, :] < lens[:, None]
    has_n = (live & (q == 255)).any(1)
    only_N = (lens > 0) & ((q == 0) | ~live).all(1)
    plain = ~has_n & ~only_N & (lens > 0)
    out = set()
    for what, m in (("row0", plain & (rows == 1)), ("rowR-1", plain & (rows == R)), ("rowR", plain & (rows == R + 1)),
                    ("onlyN", only_N), ("has_n", has_n), ("len0", lens == 0)):
        if m.any():
            out.add(("narrow", layout, R, what))
    return out


def missing(required, filled):
    return [c for c in required if c not in filled]


# ---- the generator ---------------------------------------------------------------------------------------------------

class Batch:
    """One call's input: q (n x stride), lens (always given; fixed_len is set when every read has that length and the batch
    is to be passed as a fixed-length one), alpha, and what it is for."""

    def __init__(self, name, kind, alpha, q, lens, fixed_len=None, final_cap=None):
        self.name, self.kind, self.alpha, self.q, self.lens = name, kind, float(alpha), q, lens.astype(np.int32)
        self.fixed_len, self.final_cap = fixed_len, final_cap
        self.n, self.stride = q.shape

    def len_kw(self):
        return dict(fixed_len=self.fixed_len) if self.fixed_len is not None else dict(lens=self.lens)


def _sprinkle(q, lens):
    """A few 'N' / 'n' bytes in some reads (deterministic, by position in the pool)."""
    i = np.arange(len(lens))
    for m, code, at in ((i % 9 == 4, 0, lens // 2), (i % 13 == 6, 255, lens // 3), (i % 31 == 7, 0, lens - 1)):
        m = m & (lens >= 4)
        q[i[m], at[m]] = code


def _uniform_pool(specs, stride):
    """specs: [(qa, qb, s_lo, s_hi[, step])] -> every read of S = s_lo .. s_hi bases (every step-th) that alternate between
    qualities qa and qb."""
    specs = [tuple(sp) + (1,) * (5 - len(sp)) for sp in specs]
    lens = np.concatenate([np.arange(lo, hi + 1, step) for _, _, lo, hi, step in specs]).astype(np.int32)
    q = np.zeros((len(lens), stride), np.uint8)
    at = 0
    col = np.arange(stride)
    for qa, qb, lo, hi, step in specs:
        n = len(range(lo, hi + 1, step))
        q[at:at + n] = np.where(col % 2 == 0, qa, qb)[None, :]
        at += n
    q[col[None, :] >= lens[:, None]] = 0
    _sprinkle(q, lens)
    return q, lens


def _prefix_pool(L, stride, q_lows):
    """Fixed-length reads: k bases of a low quality, then Q40, for every k = 0 .. L."""
    k = np.tile(np.arange(L + 1), len(q_lows))
    low = np.repeat(np.array(q_lows, np.uint8), L + 1)
    col = np.arange(stride)[None, :]
    q = np.where(col < k[:, None], low[:, None], np.uint8(40)).astype(np.uint8)
    q[:, L:] = 0
    lens = np.full(len(k), L, np.int32)
    _sprinkle(q, lens)
    return q, lens


def _pick(cand, cells_of, wanted, per_cell, rng, have):
    """Indices (from the candidates `cand`) of up to per_cell reads for each wanted cell; cells_of(i) -> the cells read i fills;
    `have`: cell -> count so far, updated."""
    keep = []
    for i in rng.permutation(np.asarray(cand, np.int64)):
        for c in cells_of(int(i)):
            if c in wanted and have.get(c, 0) < per_cell:
                have[c] = have.get(c, 0) + 1
                keep.append(int(i))
                break
    return sorted(set(keep))


def _first_k_per_key(idx, keys, k, rng):
    """Up to k of the indices `idx` for every distinct key, drawn at random."""
    perm = rng.permutation(len(idx))
    idx, keys = np.asarray(idx)[perm], np.asarray(keys)[perm]
    order = np.argsort(keys, kind="stable")
    ks = keys[order]
    start = np.r_[0, np.nonzero(ks[1:] != ks[:-1])[0] + 1] if len(ks) else np.zeros(0, np.int64)
    rank = np.arange(len(ks)) - np.repeat(start, np.diff(np.r_[start, len(ks)]))
    return idx[order][rank < k]


PER_CELL = 2              # reads kept per cell and alpha
SEED = 20161017


def _threads(oracle):
    return max(1, min(16, oracle.lib().pbo_max_threads()))


def _oracle_rows(oracle, q, lens, alpha, sel, mode=None):
    """(rows, nan) of the selected reads of a pool; rows = -1 for the others.  The oracle is the costly step (a read costs
    length x rows cells), so a pool is first thinned with the model to the reads that can be of use.  With a mode the rows
    are those of the mode's CPU model (oracle.filter_batch_model) and `nan` marks the reads the mode hands to the exact pass."""
    rows = np.full(len(lens), -1, np.int32)
    nan = np.zeros(len(lens), bool)
    idx = np.nonzero(sel)[0]
    if len(idx) and mode is None:
        ee, _, _, r = oracle.filter_batch(np.ascontiguousarray(q[idx]), lens=lens[idx], alpha=alpha, threads=_threads(oracle))
        rows[idx], nan[idx] = r, np.isnan(ee)
    elif len(idx):
        # the oracle hands its threads 256 reads at a time and a pool of long reads is thinned to fewer than that, so the
        # reads are dealt out here, one single-threaded call per worker (each read's result is its own: the same arrays)
        def part(sub):
            m = oracle.filter_batch_model(np.ascontiguousarray(q[sub]), mode, lens=lens[sub], alpha=alpha, threads=1)
            return sub, m.rows, m.hand
        order = idx[np.argsort(-lens[idx], kind="stable")]
        workers = _threads(oracle)
        with ThreadPoolExecutor(workers) as pool:
            for sub, r, h in pool.map(part, [order[t::workers] for t in range(workers) if t < len(order)]):
                rows[sub], nan[sub] = r, h
    return rows, nan


def _main_like(oracle, name, kind, pool, alphas, wanted, rng, mode=None):
    """One batch per alpha from `pool`: the reads the model and the oracle put into a wanted main or wide cell.  With a mode
    the crossing row is the one of the mode's CPU model, and a read the mode hands to the exact pass is never picked."""
    q, lens = pool
    out = []
    codes = np.array(sorted(c[1] * 4096 + c[2] for c in wanted if c[0] == "main"), np.int64)
    wide_rows = [c[1] for c in wanted if c[0] == "wide" and isinstance(c[1], int)]
    need_j = {c[2] + 1 for c in wanted if c[0] == "main"} | {r + 1 for r in wide_rows}
    if any(c[0] == "wide" and not isinstance(c[1], int) for c in wanted):
        need_j |= {TILE_MAX_ROWS, TILE_MAX_ROWS + 1}
    need_j = np.array(sorted(need_j | {j + 1 for j in need_j}))        # the predictor gives J or J + 1
    stats = read_stats(q, lens)
    for alpha in alphas:
        pred = rows_from_stats(stats, alpha)
        budgets = cap_of_rows(pred)
        rows, nan = _oracle_rows(oracle, q, lens, alpha, np.isin(pred, need_j), mode)
        live = ~nan & (rows >= 1)
        code = budgets.astype(np.int64) * 4096 + rows - 1
        m = live & np.isin(code, codes) & (rows <= budgets)
        idx = list(_first_k_per_key(np.nonzero(m)[0], code[m], PER_CELL, rng))
        w = live & (budgets == 0) & ((rows <= TILE_MAX_ROWS + 1) | np.isin(rows - 1, wide_rows))
        w |= live & (budgets == TILE_MAX_ROWS) & (rows == TILE_MAX_ROWS)
        cells_of = lambda i: ledger_wide(rows[i:i + 1], budgets[i:i + 1], nan[i:i + 1])
        idx += _pick(np.nonzero(w)[0], cells_of, wanted, PER_CELL, rng, {})
        if idx:
            idx = rng.permutation(sorted(set(int(i) for i in idx)))
            out.append(Batch("%s_a%g" % (name, alpha), kind, alpha, np.ascontiguousarray(q[idx]), lens[idx]))
    return out


def _generate(oracle):
    rng = np.random.default_rng(SEED)
    batches = []
    # main pass, rows of up to 960 bytes (the short-row classification): every class up to cap 512
    mixes = [(1, 10), (3, 25), (2, 40)]
    specs = [(qv, qv, 1, 960) for qv in range(1, 31)] + [(a, b, 1, 960) for a, b in mixes]
    want_short = {c for c in main_cells() if c[1] <= 512}
    batches += _main_like(oracle, "main960", "main", _uniform_pool(specs, 960), ALPHAS, want_short, rng)
    # class 1024, the tile / wide boundary and k_wide's first wave boundary: reads of 600 .. 2040 bases of Q1 .. Q3 at stride 2048
    want_long = {c for c in main_cells() if c[1] == 1024} | {c for c in WIDE_CELLS if c[1] not in (2047, 2048)}
    specs = [(1, 1, 600, 1340), (2, 2, 780, 1700), (1, 2, 700, 1500), (1, 3, 800, 1640), (2, 3, 900, 1900), (1, 4, 800, 1800),
             (3, 3, 1000, 2040), (1, 5, 900, 1900)]
    batches += _main_like(oracle, "main2048", "main", _uniform_pool(specs, 2048), ALPHAS, want_long, rng)
    # k_wide's second wave boundary: Q1 .. Q3 around J = 2048, 2049 at stride 4096
    want_far = {("wide", 2047), ("wide", 2048)}
    specs = [(1, 1, 2300, 2700), (2, 2, 2900, 3400), (3, 3, 3700, 4096), (1, 2, 2600, 3000)]
    batches += _main_like(oracle, "wide4096", "wide", _uniform_pool(specs, 4096), ALPHAS, want_far, rng)
    # overflow pass: one fixed-length batch per class with G > 1 (fixed_len + 1 rows select the class) and alpha
    want_ovf = set(overflow_cells(oracle))
    for cap, G, R in TILE_CLASSES:
        if G == 1:
            continue
        L = cap - 1
        q, lens = _prefix_pool(L, 16 * ((L + 15) // 16), (1, 2, 3, 6, 1) if cap < 256 else (1, 2, 1))   # Q1 twice: the N / n bytes fall elsewhere
        rows_wanted = np.array([c[2] for c in want_ovf if c[1] == cap and c[2] != "lane0"], np.int64)
        stats = read_stats(q, lens)
        for alpha in overflow_alphas(oracle, cap):
            full = rows_from_stats(stats, alpha)
            budgets = cap_of_rows(rows_from_stats(stats, alpha, underpredict=True))
            sel = np.isin(full, (rows_wanted[:, None] + np.arange(1, 9)[None, :]).ravel()) | ((full >= 4) & (full <= R))   # J .. J + 7
            rows, nan = _oracle_rows(oracle, q, lens, alpha, sel)
            over = (budgets > 0) & (rows > budgets) & (rows <= cap) & ~nan
            lane0 = rng.permutation(np.nonzero(over & (rows - 1 < R - 1))[0])[:PER_CELL]
            cand = np.union1d(np.nonzero(over & np.isin(rows - 1, rows_wanted))[0], lane0)
            cells_of = lambda i: ledger_overflow(rows[i:i + 1], budgets[i:i + 1], cap, nan[i:i + 1])
            idx = _pick(cand, cells_of, want_ovf, PER_CELL, rng, {})
            if idx:
                idx = rng.permutation(idx)
                batches.append(Batch("ovf%d_a%g" % (cap, alpha), "ovf", alpha, np.ascontiguousarray(q[idx]), lens[idx],
                                     fixed_len=L, final_cap=cap))
    return batches


# ---- MPB_FLAG_FAST_FMA and MPB_FLAG_ODDS: the same cells, by the mode's own crossing rows ---------------------------------

P0_MIN_LOG2 = -900                                 # ODDS' range guard: a read with p0 < 2^-900 goes to the exact pass
ODDS_LADDER_Q = tuple(range(3, 21))
LONG_STRIDE_MAX = 16384                            # only the Q16 .. Q20 pool lies above it
ODDS_FAR_MAX = 64                                  # candidates of that pool


def q_bits(qv):
    """-log2(1 - p) of a quality: what one base of it takes off log2 p0."""
    return -math.log2(1.0 - 10.0 ** (-qv / 10.0))


def odds_longest(qa, qb=None):
    """About the most bases of alternating qualities qa, qb that keep p0 >= 2^-900 (the model has the last word)."""
    per = (q_bits(qa) + q_bits(qa if qb is None else qb)) / 2
    return int(-P0_MIN_LOG2 / per)


def odds_bound(oracle):
    """B: the largest model J over the uniform reads Q3 .. Q20, each at its longest length with p0 >= 2^-900, alpha 1e-5."""
    if "B" not in _CACHE:
        def longest_j(qv):
            top = odds_longest(qv) + 2
            lens = np.arange(top - 3, top + 1).astype(np.int32)         # the float estimate of the longest length, -1 .. +2
            q = np.full((len(lens), 16 * ((top + 15) // 16)), qv, np.uint8)
            q[np.arange(q.shape[1])[None, :] >= lens[:, None]] = 0
            m = oracle.filter_batch_model(q, "odds", lens=lens, alpha=min(MODE_ALPHAS), threads=1)
            ok = ~m.hand & (m.p0 >= 2.0 ** P0_MIN_LOG2)
            assert ok[0] and not ok[-1], qv                               # the four lengths straddle the guard
            return int(m.rows[ok].max())
        with ThreadPoolExecutor(_threads(oracle)) as pool:
            _CACHE["B"] = max(pool.map(longest_j, ODDS_LADDER_Q[::-1]))
    return _CACHE["B"]


def odds_unreachable(oracle):
    """The main cells no read can fill under MPB_FLAG_ODDS: crossing row js needs J = js + 1 > B rows (odds_bound).
    The mode keeps a read only while p0 = prod (1 - p_k) >= 2^-900, that is sum -ln(1 - p_k) <= 900 ln 2 = 623.8; with
    -ln(1 - p) >= p the read's expected error count is sum p_k <= 623.8, its variance sum p_k (1 - p_k) is no larger, and J
    grows with the mean: J <= about 624 + z sqrt(624) + (z^2 - 1) / 6 = 733 at z = Phi^-1(1 - 1e-5) = 4.26, the smallest alpha
    the mode accepts.  Low error rates come closest (there -ln(1 - p) -> p and the variance -> the mean), and a read has at
    most 65535 bases, so the ladder's Q20 read is about the best there is; B is measured, not taken from this estimate."""
    B = odds_bound(oracle)
    return [c for c in main_cells() if c[2] + 1 > B]


def odds_cells(oracle):
    bad = set(odds_unreachable(oracle))
    return [c for c in main_cells() if c not in bad]


def _long_specs(quals, stride, mean_lo, per_j=4):
    """Reads of one quality (or two, alternating) up to the longest length the range guard lets through (and the stride), down
    to the length at which the expected error count is mean_lo, about per_j lengths for every J."""
    out = []
    for qa, qb in quals:
        pbar = (10.0 ** (-qa / 10.0) + 10.0 ** (-qb / 10.0)) / 2
        hi = min(stride, odds_longest(qa, qb) + 2)
        out.append((qa, qb, min(hi, int(mean_lo / pbar)), hi, max(1, int(1 / (per_j * pbar)))))
    return out


def _far_specs():
    """The Q16 .. Q20 pool: sixteen lengths below each quality's longest, three for every J."""
    out = []
    for qv in (16, 17, 18, 20):
        step = max(1, int(1 / (3 * 10.0 ** (-qv / 10.0))))
        hi = odds_longest(qv)
        out.append((qv, qv, hi - 15 * step, hi, step))
    return out


def mode_pools(mode):
    """[(name, stride, specs, caps of the cells wanted from it)] of a mode's main-pass batches."""
    short = [(qv, qv, 1, 960) for qv in range(1, 31)] + [(a, b, 1, 960) for a, b in [(1, 10), (3, 25), (2, 40)]]
    if mode == "fma":              # the exact batches' pools
        long_ = [(1, 1, 600, 1340), (2, 2, 780, 1700), (1, 2, 700, 1500), (1, 3, 800, 1640), (2, 3, 900, 1900),
                 (1, 4, 800, 1800), (3, 3, 1000, 2040), (1, 5, 900, 1900)]
        return [("main960", 960, short, (0, 512)), ("main2048", 2048, long_, (1024, 1024))]
    return [("main960", 960, short, (0, 512)),
            ("long2048", 2048, _long_specs([(3, 3), (4, 4), (5, 5), (6, 6), (3, 5), (4, 6)], 2048, 330, 2), (512, 1024)),
            ("long8192", 8192, _long_specs([(8, 8), (9, 9), (10, 10), (11, 11), (8, 10)], 8192, 480, 2), (1024, 1024)),
            ("long12288", 12288, _long_specs([(13, 13)], 12288, 560), (1024, 1024)),
            ("far65536", 65536, _far_specs(), (1024, 1024))]


def _generate_mode(oracle, mode):
    rng = np.random.default_rng(SEED + 1 + MODES.index(mode))
    cells = main_cells() if mode == "fma" else odds_cells(oracle)
    batches = []
    for name, stride, specs, (lo, hi) in mode_pools(mode):
        want = {c for c in cells if lo <= c[1] <= hi}
        batches += _main_like(oracle, "%s_%s" % (mode, name), "main", _uniform_pool(specs, stride), MODE_ALPHAS, want, rng, mode)
    return batches


_CACHE = {}


def generate(oracle, fresh=False, mode=None):
    """The directed batches (main, wide, ovf kinds); with mode "fma" or "odds", the main-pass batches of that mode (kind main).
    Cached per process; fresh=True generates again (determinism test)."""
    make = (lambda: _generate(oracle)) if mode is None else (lambda: _generate_mode(oracle, mode))
    if fresh:
        return make()
    key = "b" if mode is None else "b_" + mode
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


# ---- ODDS' range guard at its boundary, and the 1e-9 band around a read's limit ----------------------------------------------

GUARD_CORES = {384: 1, 512: 3, 1024: 10}           # class -> the quality whose longest kept read crosses in that class
GUARD_TRIM = (3, 6, 10, 13, 20, 30)                # coarse to fine: bases that bring log2 p0 to within 0.03 bit above -900
GUARD_BAND = 0.05                                  # bits: every read of a ladder lies this close to 2^-900


def range_guard_ladder(oracle, cap):
    """(q, lens, kc): reads of class `cap` whose p0 steps across 2^-900.  A core of one low quality, a few trimming bases,
    then k bases of Q40 -- each moves log2 p0 by 1.4e-4 -- for k around kc, the first k at which the float estimate of p0
    falls below the guard (the model's p0, not this estimate, says on which side a read lies)."""
    a, _ = oracle.lut()
    bits = lambda qv: -math.log2(a[qv])
    core = GUARD_CORES[cap]
    quals = [core] * int((-P0_MIN_LOG2 - 1) / bits(core))
    left = -P0_MIN_LOG2 - len(quals) * bits(core)
    for qv in GUARD_TRIM:
        k = max(0, int((left - 0.02) / bits(qv)))
        quals += [qv] * k
        left -= k * bits(qv)
    assert 0.015 < left < 0.03, left
    kc = int(left / bits(40)) + 1
    span = int((GUARD_BAND - 0.01) / bits(40)) - kc
    ks = sorted({0, kc - 64, kc - 8, kc - 3, kc - 2, kc - 1, kc, kc + 1, kc + 2, kc + 8, kc + 64, kc + span})
    lens = np.array([len(quals) + k for k in ks], np.int32)
    q = np.zeros((len(ks), 16 * ((int(lens.max()) + 15) // 16)), np.uint8)
    q[:, :len(quals)] = np.array(quals, np.uint8)[None, :]
    q[:, len(quals):] = 40
    q[np.arange(q.shape[1])[None, :] >= lens[:, None]] = 0
    return q, lens, kc


def band_batch():
    """(q, lens): 123 uniform and two-quality reads of 230 .. 330 bases at stride 336, of class 160 at alpha 0.005."""
    return _uniform_pool([(3, 3, 230, 270), (4, 4, 290, 330), (2, 5, 240, 280)], 336)


def band_picks(model, k=3):
    """Reads whose model ee (ambigs ignore, no limit near) is far from an integer -- so that --round's own band stays out of
    the way -- spread over the batch."""
    e = model.ee_model
    ok = np.flatnonzero(~model.hand & (np.abs(e - np.rint(e)) > 0.05) & (e > 100))
    return [int(i) for i in ok[:: max(1, len(ok) // k)][:k]]


BAND_FACTORS = ((0.5e-9, True), (2e-9, False))      # |limit / e - 1|, and whether the mode hands the read back there


def model_ledger_mode(oracle, batches, mode, alpha=None):
    """What a mode's batches fill under the predictor model's budgets and the mode model's rows: (main cells, thin cells)."""
    main, thin = set(), set()
    for b in batches:
        if alpha is not None and b.alpha != alpha:
            continue
        m = oracle.filter_batch_model(b.q, mode, lens=b.lens, alpha=b.alpha, threads=_threads(oracle))
        budgets = cap_of_rows(predicted_rows(b.q, b.lens, b.alpha))
        main |= ledger_mode(m, budgets)
        if b.stride <= 2048:
            thin |= ledger_thin_mode(m, budgets)
    return main, thin


def model_ledger(oracle, batches):
    """What the batches fill under the model's budgets and the oracle's rows: (main + wide + thin cells, overflow cells)."""
    filled = set()
    for b in batches:
        ee, _, _, rows = oracle.filter_batch(b.q, lens=b.lens, alpha=b.alpha, threads=_threads(oracle))
        nan = np.isnan(ee)
        if b.kind == "ovf":
            budgets = cap_of_rows(predicted_rows(b.q, b.lens, b.alpha, underpredict=True))
            filled |= ledger_overflow(rows, budgets, b.final_cap, nan)
        else:
            budgets = cap_of_rows(predicted_rows(b.q, b.lens, b.alpha))
            filled |= ledger_main(rows, budgets, nan) | ledger_wide(rows, budgets, nan)
            if b.stride <= 2048:
                filled |= ledger_thin(rows, budgets, nan)
    return filled


# ---- narrow forms and sub-views: 10,000 reads, mostly clean, with the directed reads in fixed places ------------------

NARROW_N = 10_000


def narrow_batch(oracle, layout):
    """(q, lens, fixed_len or None) for a layout of NARROW_LAYOUTS: the clean synthetic profile (nearly every read crosses on its
    second row) with, every 50 reads, a read of one quality throughout -- Q70 down to Q12, so that the crossing row runs from 0
    to far beyond four --, reads of only 'N', reads with an 'n', and (ragged) reads of no bases."""
    stride = int(layout[-3:])
    ragged = layout.startswith("ragged")
    if ragged:
        q, lens = oracle.synth_fill(NARROW_N, stride, min_len=50, max_len=600, seed=6, profile=1)
    else:
        q, lens = oracle.synth_fill(NARROW_N, stride, fixed_len=300, seed=2, profile=1)
    q = q.copy()
    lens = lens.astype(np.int32).copy()
    col = np.arange(stride)[None, :]
    k = 0
    for i in range(7, NARROW_N, 50):
        q[i, :] = 70 - (k % 59)                       # Q70 .. Q12
        k += 1
    q[11::500, :] = 0                                  # only 'N'
    q[13::97, 5] = 255                                 # an 'n'
    q[17::89, 3] = 0                                   # an 'N' in an otherwise clean read
    if ragged:
        lens[19::1000] = 0
        lens[23::1000] = 1
        lens[29::1000] = 600
        q[col >= lens[:, None]] = 0
    else:
        q[:, 300:] = 0
    return q, lens, (None if ragged else 300)
