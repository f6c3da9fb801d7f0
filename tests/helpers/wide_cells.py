"""Directed inputs for k_wide (moira_amd/csrc/mpb_kernels.hip), the kernel of every read that needs more than 1024 DP rows: which
cells a batch must reach, a generator that reaches them, and the ledger that says which were reached.  Plain Python and numpy;
no GPU.  (class_cells.py's WIDE_CELLS stop at the first two wave boundaries of the main pass.)

k_wide is compiled eight times -- FINAL (the overflow pass: every read gets len + 1 rows) x W in {2, 4, 8, 16} waves per
workgroup -- and a read of nw = ceil(rows / 1024) waves is taken by the instance W_of(nw).  The places with code of their own:

  boundary  ("wide", pass, w, side): the CDF crosses in the last row of wave w - 1 (side "last": J = 1024 w rows, js = 1024 w - 1,
            lane 63, row 15) or in the first row of wave w (side "first": J = 1024 w + 1, lane 0, row 0, the running sum taken
            from the wave before), w = 1 .. 15; ("wide", "main", 16, "last") is the last supported row, J = 16384, and
            ("wide", "main", "beyond") a read of J = 16385, which has no result in either pass
  edge      ("wide", "main", "edge", b): a read PREDICTED at exactly b rows and one at b + 1, b in {2048, 4096, 8192} -- the last
            read of the instance W and the first of 2 W; ("wide", "final", "edge", b): reads of b - 1 and of b bases
  trailing  ("wide", "main", "trailing"): the crossing wave is not the read's last active wave (the waves behind it go through
            the found0 branch of the epilogue); in the final pass this is every read but the "lastwave" ones
  final     ("wide", "final", "nw1"): a read of fewer than 1024 bases in the overflow list of a long batch (the W = 2
            instance's extra duty); ("wide", "final", "lastwave", W), W in {2, 4}: a crossing in the last active wave
  block     ("wide", pass, "block", r), r = li % 64 in {63, 0, 1}, on a read of nw >= 3 (the prefetch bound nb0 < li, nblk,
            nsteps = nblk + nw - 1), and ("wide", pass, "full_row"): li = the row stride; every row's padding is random bytes
  ambiguity ("wide", pass, "N_run"): a run of byte 0 across a 64-base block edge; "N_last": byte 0 at position li - 1;
            "n": one byte 255 in a read of nw >= 3
  trips     ("wide", pass, "trips"): the list of the pass holds at least 2049 reads -- with MPB_WIDE_GRID = 1024 workgroups every
            one of them then makes two trips of the list loop whatever the list's order --, at least 400 of them of nw <= 2 and
            at least 400 of nw = 3 or 4, so that an instance steps over another's reads between two of its own

Which model a read's nw comes from.  The library reports no budget for a wide read (mpb_last_read_budgets gives 0), so the nw
of a main-pass cell is the float64 model's (front_end_model.x64), and a read counts only if it is SURE: both ends of the band
BAND_ABS + BAND_REL |x| give the same ceil(rows / 1024) -- for an "edge" cell the same row count.  That figure only decides what
a batch claims to cover; what the GPU tests assert is the oracle's result.  In the final pass nw = min(16, ceil((li + 1) / 1024))
is exact; a read is in that pass's list when its halved budget provably misses: a sure tile budget below J, or a sure wide
read with J > 1024 nw.
"""
import math
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from helpers import front_end_model as FE
from helpers.class_cells import Batch, cap_of_rows, inv_norm_cdf

WIDE_WAVES, WIDE_R, WIDE_GRID = 16, 16, 1024             # MPB_WIDE_WAVES, MPB_WIDE_R, MPB_WIDE_GRID
WAVE_ROWS = 64 * WIDE_R                                  # rows of one wave
MAX_ROWS = WAVE_ROWS * WIDE_WAVES                        # 16384: the most rows a read may need
INSTANCES = (2, 4, 8, 16)
EDGES = (2048, 4096, 8192)
ALPHA, ALPHA_B = 0.005, 0.05                             # the whole ladder; w <= 4 once more
SEED = 20161019
PASSES = ("main", "final")
TRIPS_MIN, TRIPS_EACH = 2 * WIDE_GRID + 1, 400


def W_of(nw):
    """The instance that takes a read of nw waves: the kernel's filter `nw > W || (W > 2 && nw <= W / 2)` skips it elsewhere."""
    return 2 if nw <= 2 else 4 if nw <= 4 else 8 if nw <= 8 else 16


def kernel_takes(W, nw):
    """The filter as the kernel states it."""
    return not (nw > W or (W > 2 and nw <= W // 2))


def nw_of(rows):
    rows = np.asarray(rows, np.int64)
    return np.clip((rows + WAVE_ROWS - 1) // WAVE_ROWS, 1, WIDE_WAVES)


# ---- required cells --------------------------------------------------------------------------------------------------

def boundary_cells(pass_):
    return [("wide", pass_, w, side) for w in range(1, WIDE_WAVES) for side in ("last", "first")]


def required_cells():
    out = boundary_cells("main") + [("wide", "main", 16, "last"), ("wide", "main", "beyond")]
    out += [("wide", "main", "edge", b) for b in EDGES] + [("wide", "main", "trailing")]
    out += boundary_cells("final") + [("wide", "final", "edge", b) for b in EDGES]
    out += [("wide", "final", "nw1")] + [("wide", "final", "lastwave", W) for W in (2, 4)]
    for p in PASSES:
        out += [("wide", p, "block", r) for r in (63, 0, 1)] + [("wide", p, "full_row")]
        out += [("wide", p, what) for what in ("N_run", "N_last", "n")]
    return out


def trips_cells():
    return [("wide", p, "trips") for p in PASSES]


GROUPS = ("boundary", "end", "edge", "trailing", "final", "block", "ambiguity", "trips")


def group_of(cell):
    what = cell[2]
    if isinstance(what, int):
        return "boundary" if what < 16 else "end"
    return {"beyond": "end", "edge": "edge", "trailing": "trailing", "nw1": "final", "lastwave": "final", "block": "block",
            "full_row": "block", "trips": "trips"}.get(what, "ambiguity")


# ---- the model -------------------------------------------------------------------------------------------------------

class Rows:
    """The float64 model's row count of every read at x and at both ends of its band, plain or halved."""

    def __init__(self, q, lens, alpha, underpredict=False):
        x, scored = FE.x64(q, lens, alpha)
        b = FE.BAND_ABS + FE.BAND_REL * np.abs(x)
        self.rows = FE.rows_of(x, scored, underpredict)
        self.lo, self.hi = FE.rows_of(x - b, scored, underpredict), FE.rows_of(x + b, scored, underpredict)
        self.sure_rows = self.lo == self.hi
        self.nw = nw_of(self.rows)
        self.sure_wide = (self.lo > WAVE_ROWS) & (nw_of(self.lo) == nw_of(self.hi))      # wide, and of a known wave count
        self.sure_tile = (self.hi <= WAVE_ROWS) & (cap_of_rows(self.lo) == cap_of_rows(self.hi))
        self.cap = cap_of_rows(self.rows)                                                # of a sure tile read: its budget


def misses_halved(q, lens, alpha, J, budgets=None):
    """Reads whose budget under MPB_FLAG_TEST_UNDERPREDICT provably misses (they are in the final pass's list), and those that
    provably do not.  budgets: what the library reported for that run (0 = wide); without them the model's sure tile caps."""
    m = Rows(q, lens, alpha, underpredict=True)
    J = np.asarray(J, np.int64)
    if budgets is None:
        tile, cap = m.sure_tile, m.cap.astype(np.int64)
        wide = m.sure_wide
    else:
        budgets = np.asarray(budgets, np.int64)
        tile, cap = budgets > 0, budgets
        wide = (budgets == 0) & m.sure_wide
    miss = (tile & (J > cap)) | (wide & (J > WAVE_ROWS * m.nw))
    holds = (tile & (J <= cap)) | (wide & (J <= WAVE_ROWS * m.nw))
    return miss, holds


# ---- the ledger ------------------------------------------------------------------------------------------------------

def _ambiguity(q, lens):
    """(N_run, N_last, one_n) per read, from the bytes before each read's length."""
    q, lens = np.asarray(q), np.asarray(lens)
    n, stride = q.shape
    col = np.arange(stride)[None, :]
    live = col < lens[:, None]
    zero = live & (q == 0)
    run = np.zeros(n, bool)
    if stride > 64:
        run = (zero[:, 63:-1:64] & zero[:, 64::64]).any(1)
    last = np.zeros(n, bool)
    has = lens > 0
    last[has] = q[np.nonzero(has)[0], lens[has] - 1] == 0
    return run, last, (live & (q == 255)).sum(1) == 1


def ledger(b, J, nan=None, budgets=None, budgets_under=None):
    """Cells the batch b fills, from the oracle's rows J.  budgets / budgets_under: what the library reported for the plain and
    the underpredicted run (0 = wide); without them the model decides which reads are wide.  Sub-cells ("edge", b, 0 | 1) are
    folded into their cell by fold()."""
    J = np.asarray(J, np.int64)
    lens = b.lens.astype(np.int64)
    nan = np.zeros(b.n, bool) if nan is None else np.asarray(nan)
    run, last, one_n = _ambiguity(b.q, b.lens)
    out = set()
    # main pass: sure wide reads (that the library lists as wide too)
    m = Rows(b.q, b.lens, b.alpha)
    wide = m.sure_wide if budgets is None else m.sure_wide & (np.asarray(budgets) == 0)
    crossed = wide & (J <= WAVE_ROWS * m.nw) & ~nan                # crosses inside the waves the main pass runs
    # final pass: reads that provably miss their halved budget, in a batch whose overflow pass is the wide kernel
    miss, _ = misses_halved(b.q, b.lens, b.alpha, J, budgets_under)
    final = miss & (b.stride > WAVE_ROWS - 1)
    nwf = nw_of(lens + 1)
    for p, sel, nw in (("main", crossed, m.nw), ("final", final & ~nan & (J <= MAX_ROWS), nwf)):
        for i in np.nonzero(sel)[0]:
            j, w, k = int(J[i]), int(J[i]) // WAVE_ROWS, int(nw[i])
            if j % WAVE_ROWS == 0 and (w <= 15 or p == "main"):
                out.add(("wide", p, w, "last"))
            if j % WAVE_ROWS == 1 and 1 <= w <= 15:
                out.add(("wide", p, w, "first"))
            if p == "main" and (j - 1) // WAVE_ROWS < k - 1:
                out.add(("wide", "main", "trailing"))
            if p == "final" and (j - 1) // WAVE_ROWS == k - 1 and k in (2, 4):
                out.add(("wide", "final", "lastwave", k))
            if p == "final" and lens[i] < WAVE_ROWS:
                out.add(("wide", "final", "nw1"))
            if k >= 3 and lens[i] % 64 in (63, 0, 1):
                out.add(("wide", p, "block", int(lens[i] % 64)))
            if k >= 2 and lens[i] == b.stride:
                out.add(("wide", p, "full_row"))
            if run[i]:
                out.add(("wide", p, "N_run"))
            if last[i]:
                out.add(("wide", p, "N_last"))
            if one_n[i] and k >= 3:
                out.add(("wide", p, "n"))
    for e in EDGES:
        for side in (0, 1):
            if (crossed & m.sure_rows & (m.rows == e + side)).any():
                out.add(("wide", "main", "edge", e, side))
            if (final & (lens + 1 == e + side)).any():
                out.add(("wide", "final", "edge", e, side))
    # a read of more than 16384 rows: listed wide, never crossing, NaN after the final pass
    if (wide & (m.lo > MAX_ROWS) & (J == MAX_ROWS + 1) & (lens + 1 > MAX_ROWS)).any():
        out.add(("wide", "main", "beyond"))
    return out


def ledger_trips(b, J, budgets=None, budgets_under=None):
    """The list cells: the main pass's list is the batch's (sure) wide reads, the final pass's the reads that provably miss."""
    out = set()
    m = Rows(b.q, b.lens, b.alpha)
    wide = m.sure_wide if budgets is None else m.sure_wide & (np.asarray(budgets) == 0)
    miss, _ = misses_halved(b.q, b.lens, b.alpha, J, budgets_under)
    miss = miss & (b.stride > WAVE_ROWS - 1)
    for p, sel, nw in (("main", wide, m.nw), ("final", miss, nw_of(b.lens.astype(np.int64) + 1))):
        if sel.sum() >= TRIPS_MIN and (sel & (nw <= 2)).sum() >= TRIPS_EACH and (sel & (nw >= 3) & (nw <= 4)).sum() >= TRIPS_EACH:
            out.add(("wide", p, "trips"))
    return out


def fold(cells):
    """Edge cells need both their reads."""
    out = {c for c in cells if not (c[2] == "edge" and len(c) == 5)}
    for p in PASSES:
        for e in EDGES:
            if ("wide", p, "edge", e, 0) in cells and ("wide", p, "edge", e, 1) in cells:
                out.add(("wide", p, "edge", e))
    return out


def missing(required, filled):
    return [c for c in required if c not in filled]


# ---- the committed length table ----------------------------------------------------------------------------------------

# (alpha, J) -> (bases, k, tail): a read of `bases` bases of Q1 whose first k bases are Q2, followed by `tail` bases of Q40, needs J
# rows at that alpha (the oracle's rows), and the model is sure of its predicted row count and calls it wide.  Found once by
# search_ladder(); test_wide_cells.py checks that the table reproduces its J.  One more base of Q1 raises J by 0 or 1, so every
# J is met; a base of Q2 for one of Q1 moves the predictor's x by -0.16 and takes a read whose x lies inside the band of a
# rounding step out of it.  The predictor is good: on these reads J steps where x passes a half (x = 1023.522 for J = 1024 ->
# 1025 at alpha 0.005), so the predicted rows are J, and a WIDE read of J = 1024 -- predicted at 1025: the one read here whose
# crossing wave is not its last -- has x between 1023.5 + the band (0.0202) and that step; bases of Q40 (1.1e-5 each) reach it.
# At alpha 0.05 the step lies at 1023.506, inside the band: no read of J = 1024 is surely wide there, and the second ladder
# starts at J = 1025.
LADDER = {
    (0.05, 1025): (1260, 0, 0), (0.05, 2048): (2535, 0, 0), (0.05, 2049): (2536, 0, 0), (0.05, 3072): (3815, 0, 0),
    (0.05, 3073): (3816, 0, 0), (0.05, 4096): (5096, 0, 0), (0.05, 4097): (5097, 0, 0),
    (0.005, 1024): (1243, 0, 156), (0.005, 1025): (1244, 0, 0), (0.005, 2047): (2511, 0, 0), (0.005, 2048): (2512, 0, 0),
    (0.005, 2049): (2513, 0, 0), (0.005, 3072): (3786, 0, 0), (0.005, 3073): (3787, 0, 0), (0.005, 4095): (5061, 0, 0),
    (0.005, 4096): (5063, 0, 0), (0.005, 4097): (5064, 0, 0), (0.005, 5120): (6341, 0, 0), (0.005, 5121): (6342, 0, 0),
    (0.005, 6144): (7620, 0, 0), (0.005, 6145): (7621, 0, 0), (0.005, 7168): (8900, 0, 0), (0.005, 7169): (8901, 0, 0),
    (0.005, 8191): (10179, 0, 0), (0.005, 8192): (10180, 0, 0), (0.005, 8193): (10182, 0, 0), (0.005, 9216): (11461, 0, 0),
    (0.005, 9217): (11463, 0, 0), (0.005, 10240): (12743, 0, 0), (0.005, 10241): (12744, 0, 0), (0.005, 11264): (14025, 0, 0),
    (0.005, 11265): (14026, 0, 0), (0.005, 12288): (15307, 0, 0), (0.005, 12289): (15308, 0, 0), (0.005, 13312): (16589, 0, 0),
    (0.005, 13313): (16591, 0, 0), (0.005, 14336): (17872, 0, 0), (0.005, 14337): (17873, 0, 0), (0.005, 15360): (19155, 0, 0),
    (0.005, 15361): (19156, 0, 0), (0.005, 16384): (20438, 0, 0), (0.005, 16385): (20440, 1, 0),
}
TAIL_STEP, TAIL_MAX = 4, 400                             # the Q40 tails the search tries


def ladder_targets(alpha):
    """The J a ladder must hold: both sides of every wave boundary, the end of the range, and around every instance edge."""
    top = WIDE_WAVES if alpha == ALPHA else 4
    js = set()
    for w in range(1, top + 1):
        js |= {WAVE_ROWS * w, WAVE_ROWS * w + 1}
        if WAVE_ROWS * w in EDGES and alpha == ALPHA:
            js.add(WAVE_ROWS * w - 1)
    if alpha != ALPHA:
        js.discard(WAVE_ROWS)                            # (see LADDER)
    return sorted(js)


def ladder_read(bases, k, tail=0, stride=None):
    """The row of a table entry (bases + tail bytes, or `stride` bytes: the Q1 part then runs on to the row's end)."""
    row = np.ones(bases + tail if stride is None else stride, np.uint8)
    row[:k] = 2
    if tail:
        row[bases:bases + tail] = 40
    return row


def _x_uniform(bases, alpha, p=10 ** -0.1):
    z = inv_norm_cdf(1 - alpha)
    return p * bases + z * math.sqrt(p * (1 - p) * bases) + (1 - 2 * p) * (z * z - 1) / 6


def _deal(oracle, q, lens, alpha, workers=8):
    """The oracle's rows of a few long reads: one single-threaded call per worker, longest first (class_cells._oracle_rows)."""
    rows = np.zeros(len(lens), np.int32)
    nan = np.zeros(len(lens), bool)
    order = np.argsort(-np.asarray(lens), kind="stable")

    def part(sub):
        ee, _, _, r = oracle.filter_batch(np.ascontiguousarray(q[sub]), lens=lens[sub], alpha=alpha, threads=1)
        return sub, r, np.isnan(ee)
    with ThreadPoolExecutor(workers) as pool:
        for sub, r, h in pool.map(part, [order[t::workers] for t in range(workers) if t < len(order)]):
            rows[sub], nan[sub] = r, h
    return rows, nan


def search_ladder(oracle, alpha, targets=None, max_k=6):
    """{J: (bases, k, tail)} for the targets: thirteen consecutive lengths of Q1 around the length whose x is the target, the
    oracle on each; a read whose model row count is not sure (or not wide) is tried again with k = 1 .. max_k bases of Q2 (on its
    own length and the next two, since a swap may take a row off J), and last with tails of Q40.  This reproduces LADDER; the
    whole of it costs a minute of oracle time, so no test runs more than its cheapest windows."""
    targets = ladder_targets(alpha) if targets is None else targets
    out = {}
    for centre in sorted({int(round(j / WAVE_ROWS)) * WAVE_ROWS for j in targets}):
        near = [j for j in targets if abs(j - centre) <= 1]
        L0 = next(L for L in range(1, 70000) if _x_uniform(L, alpha) >= centre - 1)
        lengths = np.arange(L0 - 6, L0 + 7)
        found_at = []
        tries = [(k, 0) for k in range(max_k + 1)] + [(0, t) for t in range(TAIL_STEP, TAIL_MAX + 1, TAIL_STEP)]
        for k, tail in tries:
            todo = [j for j in near if j not in out]
            if not todo:
                break
            stride = 16 * ((int(lengths.max()) + tail + 15) // 16)
            q = np.stack([ladder_read(int(L), k, tail, stride) for L in lengths])
            lens = (lengths + tail).astype(np.int32)
            m = Rows(q, lens, alpha)
            good = m.sure_rows & (m.lo > WAVE_ROWS)             # sure of its rows, and wide
            # after the first round only the lengths that can still be of use: at or just above one that gave a wanted J
            idx = np.arange(len(lens))
            if k or tail:
                idx = np.nonzero(good & np.isin(lengths, [L + d for L in found_at for d in ((0, 1, 2) if k else (0,))]))[0]
            if not len(idx):
                continue
            rows, _ = _deal(oracle, q[idx], lens[idx], alpha)
            if not (k or tail):
                found_at = [int(L) for L, r in zip(lengths, rows) if r in todo]
            for i, r in zip(idx, rows):
                if int(r) in todo and int(r) not in out and good[i]:
                    out[int(r)] = (int(lengths[i]), k, tail)
    return out


# ---- the generator ---------------------------------------------------------------------------------------------------

STRIDES = (5248, 10496, 20736)                      # rows of up to 4, 8 and 16 waves of Q1 (a multiple of 16 each)
STRIDE_ROWS = (4097, 8193, 16385)                   # the largest J of each
BATCH_NAMES = tuple("wide%d_a%g" % (s, ALPHA) for s in STRIDES) + ("wide%d_a%g" % (STRIDES[0], ALPHA_B),)
SMALL_ROWS = 4096                                 # the sub-batch the modes and arithmetics are compared on


def _pad(rng, q, lens):
    """Random bytes, 0 and 255 among them, behind every read's end (front_end_model.family_q leaves such rows too)."""
    junk = rng.integers(0, 256, q.shape).astype(np.uint8)
    dead = np.arange(q.shape[1])[None, :] >= np.asarray(lens)[:, None]
    q[dead] = junk[dead]


def _batch(name, alpha, stride, reads, rng):
    """reads: [(row bytes, length)] -> Batch, in a random order, padded."""
    order = rng.permutation(len(reads))
    q = np.zeros((len(reads), stride), np.uint8)
    lens = np.zeros(len(reads), np.int32)
    for at, i in enumerate(order):
        row, L = reads[i]
        q[at, :L] = row[:L]
        lens[at] = L
    _pad(rng, q, lens)
    return Batch(name, "wide", alpha, q, lens)


def _extras():
    """The reads no search is needed for: [(row, length)] at stride STRIDES[0], alpha ALPHA."""
    s = STRIDES[0]
    out = [(ladder_read(L, 0), L) for L in (2047, 2048, 4095, 4096, 4097, 600, 0)]      # final edges, lastwave, block 63 / 0 / 1, nw1
    out.append((ladder_read(s, 0), s))                                                  # full_row
    a = ladder_read(4000, 0)
    a[120:136] = 0                                                                      # N_run over the block edge at 128
    a[1023:1025] = 0                                                                    # ... and the one at 1024
    b = ladder_read(3990, 0)
    b[3989] = 0                                                                         # N_last
    c = ladder_read(4010, 0)
    c[2500] = 255                                                                       # n
    d = ladder_read(3500, 0)
    d[::3] = 3                                                                          # a mixed profile
    d[700] = 255
    d[3499] = 0
    return out + [(a, 4000), (b, 3990), (c, 4010), (d, 3500)]


def _generate():
    rng = np.random.default_rng(SEED)
    reads = {s: [] for s in STRIDES}
    for (alpha, J), (L, k, tail) in sorted(LADDER.items()):
        if alpha != ALPHA:
            continue
        s = next(s for s, top in zip(STRIDES, STRIDE_ROWS) if L + tail <= s and J <= top)
        reads[s].append((ladder_read(L, k, tail), L + tail))
    reads[STRIDES[0]] += _extras()
    reads[STRIDES[1]] += [(ladder_read(L, 0), L) for L in (8191, 8192)]                 # final edge 8192
    out = [_batch("wide%d_a%g" % (s, ALPHA), ALPHA, s, reads[s], rng) for s in STRIDES]
    second = [(ladder_read(L, k, tail), L + tail) for (alpha, J), (L, k, tail) in sorted(LADDER.items()) if alpha == ALPHA_B]
    out.append(_batch("wide%d_a%g" % (STRIDES[0], ALPHA_B), ALPHA_B, STRIDES[0], second, rng))
    assert tuple(b.name for b in out) == BATCH_NAMES
    return out


_CACHE = {}


def generate(fresh=False):
    """The directed batches: the ladder of LADDER and the extra reads, one batch per stride (and one for the second alpha)."""
    if fresh:
        return _generate()
    if "b" not in _CACHE:
        _CACHE["b"] = _generate()
    return _CACHE["b"]


def oracle_results(oracle, b, workers=8, **kw):
    """(ee, ns, pass, rows) of a directed batch: the reads dealt out one single-threaded call per worker, longest first."""
    ee, ns = np.zeros(b.n), np.zeros(b.n, np.int32)
    ps, rows = np.zeros(b.n, np.uint8), np.zeros(b.n, np.int32)
    order = np.argsort(-b.lens, kind="stable")

    def part(sub):
        return sub, oracle.filter_batch(np.ascontiguousarray(b.q[sub]), lens=b.lens[sub], alpha=b.alpha, threads=1, **kw)
    with ThreadPoolExecutor(workers) as pool:
        for sub, r in pool.map(part, [order[t::workers] for t in range(workers) if t < len(order)]):
            ee[sub], ns[sub], ps[sub], rows[sub] = r
    return ee, ns, ps, rows


def small_part(b, rows):
    """The reads of at most SMALL_ROWS rows of a batch, as a batch of its own (modes, round_ and the other arithmetics)."""
    keep = np.nonzero(np.asarray(rows) <= SMALL_ROWS)[0]
    return Batch(b.name + "_small", b.kind, b.alpha, np.ascontiguousarray(b.q[keep]), b.lens[keep]), keep


# ---- the list batch ----------------------------------------------------------------------------------------------------

LIST_STRIDE = 3008
LIST_SHORT, LIST_LONG, LIST_CLEAN, LIST_MID = 1660, 420, 300, 1100     # reads of nw <= 2, of nw = 3, clean and middling 300-base reads
LIST_SHORT_LEN, LIST_LONG_LEN = (1500, 1560), (2950, 3000)
LIST_MID_ROWS = 64                                           # a middling read needs fewer rows than this


def list_batch():
    """More than 2048 wide reads, all different -- random Q1 / Q2 bytes, about 1 % byte 0, a few 255 -- of two length groups in
    random order (nw = 2 and nw = 3: the W = 2 and W = 4 instances step over each other's reads), and between them one read of
    no bases, a few hundred clean 300-base reads (Q30 .. Q40: in no list of the plain run) and a few hundred middling ones
    (Q8 .. Q15: tile reads whose halved budget misses, so the FINAL pass's list holds them, as reads of one wave).  A clean or
    middling read the model is not sure of (plain or halved) is drawn again.

    Why the middling reads: what a workgroup keeps from its last read -- v[], the LDS stream -- is a distribution over that read's
    rows.  The next read's bases move that mass up by the next read's own expected errors, more than 1000 rows for a wide read,
    which is more than 10 sigma beyond the next read's crossing row: after a WIDE read nothing stale ever reaches a row that
    counts (the products underflow to exactly 0), so in the main pass's list no input can tell whether state was reset.  After a
    read of a few dozen rows it does: the mass lands on the next read's crossing row.  There are more middling reads than
    workgroups, so whatever order the FINAL pass's list has, some workgroup of the W = 2 instance takes two of them, and the read
    it takes after the first is one whose result stale state would change."""
    if "list" in _CACHE:
        return _CACHE["list"]
    rng = np.random.default_rng(SEED + 1)
    n = LIST_SHORT + LIST_LONG + LIST_CLEAN + LIST_MID + 1
    kind = rng.permutation(np.r_[np.zeros(LIST_SHORT, np.int8), np.ones(LIST_LONG, np.int8), np.full(LIST_CLEAN, 2, np.int8), 3,
                                 np.full(LIST_MID, 4, np.int8)])
    lens = np.where(kind == 0, rng.integers(LIST_SHORT_LEN[0], LIST_SHORT_LEN[1] + 1, n),
                    np.where(kind == 1, rng.integers(LIST_LONG_LEN[0], LIST_LONG_LEN[1] + 1, n), 300)).astype(np.int32)
    lens[kind == 3] = 0
    q = rng.integers(1, 3, (n, LIST_STRIDE)).astype(np.uint8)
    r = rng.random((n, LIST_STRIDE), np.float32)
    q[r < 0.01] = 0
    q[r > 0.9995] = 255
    redo = (kind == 2) | (kind == 4)
    for _ in range(20):
        if not redo.any():
            break
        lo = np.where(kind == 2, 30, 8)[redo]
        hi = np.where(kind == 2, 41, 16)[redo]
        q[redo] = (lo[:, None] + rng.random((int(redo.sum()), LIST_STRIDE)) * (hi - lo)[:, None]).astype(np.uint8)
        q[redo & (np.arange(n) % 7 == 0), 17] = 0
        redo &= ~(Rows(q, lens, ALPHA).sure_tile & Rows(q, lens, ALPHA, underpredict=True).sure_tile)
    assert not redo.any()
    _pad(rng, q, lens)
    b = Batch("wide_list", "list", ALPHA, q, lens)
    b.group = kind
    _CACHE["list"] = b
    return b


def list_expect(b, J):
    """(n_overflow of the plain run, of the underpredicted run), and the conditions the batch must meet -- asserted here from the
    oracle's rows and the model: every long read is surely wide and crosses inside its waves, every other read is a sure tile
    read; halved, every long read provably misses and every other read provably misses or provably holds."""
    J = np.asarray(J, np.int64)
    long_ = b.group <= 1
    m = Rows(b.q, b.lens, b.alpha)
    assert (m.sure_wide == long_).all() and (m.sure_tile == ~long_).all()
    assert (m.nw[b.group == 0] == 2).all() and (m.nw[b.group == 1] == 3).all()
    plain = int((long_ & (J > WAVE_ROWS * m.nw)).sum() + (~long_ & (J > m.cap)).sum())
    miss, holds = misses_halved(b.q, b.lens, b.alpha, J)
    assert (miss | holds).all() and miss[long_].all()
    mid = b.group == 4
    assert miss[mid].all() and (J[mid] < LIST_MID_ROWS).all() and (J[mid] > 8).all() and mid.sum() > WIDE_GRID
    return plain, int(miss.sum())
