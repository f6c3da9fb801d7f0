"""Directed inputs for the multi-block walk of the natural-order narrow pass (k_narrow, k_narrow_rs, k_narrow_rg and their one-FMA
twins k_odds_nar*; moira_amd/csrc/mpb_kernels.hip and the three mpb_narrow_*.inc bodies): the kernel instances the entry can reach,
the arithmetic of the persistent grid, a generator of small batches, and the ledger that says which cells a batch fills.  Plain
Python and numpy; no GPU.

Every instance is a persistent kernel: wave gw of W walks the row blocks (stream blocks) gw, gw + W, ... and appends the reads it
cannot finish to a segment of its own, which starts at per_blk * (gw * (nblk / W) + min(gw, nblk % W)); the ragged pass cuts the
length-sorted groups into one range per wave.  The library sizes the grid as one wave per block up to several thousand waves, so a
batch of a few thousand reads never makes a wave walk a second block; MPB_NARROW_GRID_BLOCKS (include/moira_pb.h) caps the grid's
workgroups, and the same batch then runs on three grids:
  cap1     one workgroup, W = 4: fixed shapes have 29 blocks, so wave 0 walks 8 and the others 7, nblk % W = 1
  cap3     three workgroups, W = 12: waves 0 .. 4 walk 3 blocks, the others 2, nblk % W = 5
  control  no cap: ceil(29 / 4) = 8 workgroups, every wave at most one block, waves 29 .. 31 idle

A cell is a thing that must have happened in some wave's walk for the walk to count as tested (required_fixed / required_ragged);
a ledger fills cells from the oracle's `rows` (or the odds model's) and this file's plan arithmetic alone, never from a device
result.  tests/test_narrow_walk_inputs.py asserts that no required cell stays empty; tests/test_gpu_narrow_walk.py runs the batches.

Fixed-length batches: n = 29 * per_blk - 37 reads (per_blk = 64 reads per lane's k; 37 is odd, so with two reads per lane the last
read is a lane's first and its partner lies past the end).  Each block draws a pattern -- none (no read handed back, whatever the
row count R = 2 .. 4), all (every read handed back) or mixed -- and each read a role: a target crossing row J = 1 .. 5 (scores
tuned to the length: a read of L bases of error probability p has about Poisson(L p) errors, and J is settled by L p), a read of
many rows, an 'N' (byte 0) at the first base, the last base or the last byte before a 16-byte chunk border, or an 'n' (byte 255:
always handed back).  One batch serves R = 2, 3, 4 and the twins: the ledger is taken per instance.

Ragged batches: n = 4 * 4096 + 1000 = 17,384 reads (five sort windows, n % 64 = 40), lengths uniform over the shape's range, with
two plants that keep every length valid: a hundred reads of length 0 in the second window where the range starts at 0 (one whole
group of them: they sort first), and sixteen pairs of neighbouring groups of which the first is handed back whole (an 'n' in every
read) and the second not at all (Q58 .. Q60).  rag_order() is the model of k_rag_sort: a stable sort by ceil(len / 16) >> key_shift
inside windows of 4096, 64 consecutive entries a group.  Where a wave's range ends is NOT modelled (rg_first_group balances costs);
the ragged cells that need two neighbouring groups in ONE wave are claimed by counting: W waves have W - 1 cuts, so of W or more
disjoint neighbouring pairs at least one is not cut.  The same argument gives the window border: five windows have four interior
borders, cap1 has three cuts, so some wave's range contains a border (its window base changes mid-walk)."""
import collections
import functools
import re

import numpy as np

SEED = 20261019
THREADS = 16
GRIDS = {"cap1": 1, "cap3": 3, "control": None}          # MPB_NARROW_GRID_BLOCKS per grid
CAPPED = ("cap1", "cap3")                                 # the grids with required cells
NBLK = 29                                                 # blocks of every fixed-length batch
SHORT = 37                                                # reads the last block lacks
RG_WIN, GROUP, CHUNK = 4096, 64, 16
RAGGED_N = 4 * RG_WIN + 1000
MIN_CU_BLOCKS = 256                                       # workgroups the library's own cap allows at least (one per CU, 256 CUs)
PAIRS_PLANTED = 16

Instance = collections.namedtuple("Instance", "family R RLO k odds")      # family: ring / rs / rg; k: reads per lane (rs only)


def _instances():
    out = []
    for odds in (False, True):
        out += [Instance("ring", R, R, None, odds) for R in (3, 4)]
        out += [Instance("rs", R, R, k, odds) for k in (1, 2) for R in (2, 3, 4)]
        out += [Instance("rs", 2, 2, k, odds) for k in (4, 8)]
        out += [Instance("rg", R, R, None, odds) for R in (2, 3, 4)]
    return out + [Instance("rg", R, R - 1, None, False) for R in (3, 4)]


INSTANCES = _instances()


def name_of(inst):
    return "%s%s_R%d%s%s" % ("odds_" if inst.odds else "", inst.family, inst.R, "" if inst.RLO == inst.R else "lo%d" % inst.RLO,
                             "" if inst.k is None else "_k%d" % inst.k)


def kernel_of(inst):
    """The instance's kernel as the launch tables spell it."""
    if inst.family == "ring":
        return "%s<%d, MPB_NAR_DEPTH>" % ("k_odds_nar" if inst.odds else "k_narrow", inst.R)
    if inst.family == "rs":
        return "%s<%d, %s>" % ("k_odds_nar_rs" if inst.odds else "k_narrow_rs", inst.R, "true" if inst.k <= 2 else "false")
    return "k_odds_nar_rg<%d>" % inst.R if inst.odds else "k_narrow_rg<%d, %d>" % (inst.R, inst.RLO)


# the kernels the launch tables hold and no call reaches, with the reason (test_narrow_walk_inputs.py pins this list)
UNREACHABLE = {
    "k_narrow<2, MPB_NAR_DEPTH>": "the entry takes row strides that are multiples of 16 up to 65536 only, and at two rows every such "
                                  "stride takes k_narrow_rs (nar_rs_reads_per_lane gives 1, 2, 4 or 8 reads per lane)",
    "k_odds_nar<2, MPB_NAR_DEPTH>": "the one-FMA twin of k_narrow<2>: the same dispatch, the same reason",
}

FIXED_SHAPES = {
    ("ring", None): [(300, 304), (100, 112), (17, 48), (1000, 1008)],
    ("rs", 1): [(128, 128), (65, 128), (200, 384), (30, 1024)],
    ("rs", 2): [(64, 64), (63, 64), (100, 192), (300, 320), (10, 320)],
    ("rs", 4): [(17, 32), (90, 96)],
    ("rs", 8): [(1, 16), (16, 16), (65, 80), (300, 304), (301, 304)],
}
# (lo, hi, stride, narrow_split of the mixed forms); the last one sorts with key_shift = 3 and claims the counting cells only
RAGGED_SHAPES = [(0, 300, 320, 10), (50, 600, 640, 20), (0, 1000, 1008, 32), (0, 4096, 4096, 128)]


def shapes_of(inst):
    return RAGGED_SHAPES if inst.family == "rg" else FIXED_SHAPES[(inst.family, inst.k)]


# ---- the dispatch, as mpb_kernels.hip states it ----------------------------------------------------------------------------------

_RS_BODY = [r"if \(stride % (\d+) != 0 \|\| stride > \(1 << (\d+)\)\) return 0;",
            r"if \(stride % (\d+) != 0 && rows0 != (\d+)\) return 0;",
            r"int k = 1;",
            r"while \(\(k \* stride\) % (\d+) != 0\) k \*= 2;",
            r"return k;"]
_INDEX_TEXT = [("const int ri = rows0 <= 2 ? 0 : rows0 == 3 ? 1 : 2;", 2),
               ("const int rs_k = len ? 0 : nar_rs_reads_per_lane(stride, rows0);", 2),
               ("forms[stride % 64 != 0 ? 3 : ri], grid, block", 2),
               ("hipLaunchKernelGGL(forms[ri], grid, block", 2),
               ("const bool mixed = len && split_chunks > 0 && rows0 >= 3;", 1),
               ("const int rg = mixed ? ri + 2 : ri;", 1),
               ("hipLaunchKernelGGL(nar_rg_forms[rg], grid, block", 1),
               ("hipLaunchKernelGGL(nar_rg_odds_forms[ri], grid, block", 1),
               ("if (lut_odds) return launch_narrow_odds(", 1)]


def parse_sources(kern, head):
    """The dispatch of mpb_launch_narrow / launch_narrow_odds: nar_rs_reads_per_lane's constants, the six tables of kernel
    instances, whether the lines that index them read as dispatch() restates them, and the grid's constants."""
    body = re.search(r"static int nar_rs_reads_per_lane\(int64_t stride, int rows0\)\n\{\n(.*?)\n\}", kern, re.S).group(1)
    lines = [re.sub(r"\s*//.*$", "", l).strip() for l in body.splitlines()]
    got = [re.fullmatch(p, l) for p, l in zip(_RS_BODY, lines)]
    assert len(lines) == len(_RS_BODY) and all(got), lines
    tables = {}
    for text in re.findall(r"(?:\bforms\[\d\]|nar_rg_forms\[MPB_NRG_EXACT_FORMS\]|nar_rg_odds_forms\[[^\]]*\]) = \{(.*?)\};", kern, re.S):
        names = [re.sub(r"\s+", " ", k) for k in re.findall(r"k_\w+<[^>]*>", text)]
        stem = names[0].split("<")[0]
        assert stem not in tables, stem
        tables[stem] = names
    define = lambda name, src: int(re.search(r"#define\s+%s\s+(\d+)\s" % name, src).group(1))
    grid = re.search(r"static int64_t nar_grid_blocks\(int64_t nblk, int n_cu, int per_cu, int grid_cap, int \*waves\)\n\{\n(.*?)\n\}", kern, re.S).group(1)
    return {"chunk": int(got[0].group(1)), "max_stride_log2": int(got[0].group(2)), "half": int(got[1].group(1)),
            "only_rows": int(got[1].group(2)), "line": int(got[3].group(1)), "tables": tables,
            "index_text": all(kern.count(t) == c for t, c in _INDEX_TEXT),
            "max_stride": define("MPB_MAX_STRIDE", head), "max_waves": define("MPB_NAR_MAX_WAVES", head),
            "cap_max": define("MPB_NAR_GRID_CAP_MAX", head), "rg_win": define("MPB_RG_WIN", kern), "rg_bins": define("MPB_RG_BINS", kern),
            "ring_depth": define("MPB_NAR_DEPTH", kern), "rg_max_stride": define("MPB_RG_MAX_STRIDE", head),
            "grid_lines": [re.sub(r"\s+", " ", l).strip() for l in grid.splitlines()]}


GRID_LINES = ["int64_t blocks = (nblk + 3) / 4;",
              "if (blocks > (int64_t)n_cu * per_cu) blocks = (int64_t)n_cu * per_cu;",
              "if (blocks > MPB_NAR_MAX_WAVES / 4) blocks = MPB_NAR_MAX_WAVES / 4;",
              "if (grid_cap > 0 && blocks > grid_cap) blocks = grid_cap;",
              "if (blocks < 1) blocks = 1;",
              "*waves = (int)blocks * 4;",
              "return blocks;"]


def rs_reads_per_lane(P, stride, R):
    if stride % P["chunk"] or stride > (1 << P["max_stride_log2"]):
        return 0
    if stride % P["half"] and R != P["only_rows"]:
        return 0
    k = 1
    while (k * stride) % P["line"]:
        k *= 2
    return k


def dispatch(P, stride, R, ragged, split=0, odds=False):
    """-> (kernel, reads per lane or None): what a forced call launches."""
    T = P["tables"]
    ri = 0 if R <= 2 else 1 if R == 3 else 2
    if ragged:
        if odds:
            return T["k_odds_nar_rg"][ri], None
        return T["k_narrow_rg"][ri + 2 if split > 0 and R >= 3 else ri], None
    k = rs_reads_per_lane(P, stride, R)
    if k:
        return T["k_odds_nar_rs" if odds else "k_narrow_rs"][3 if stride % 64 else ri], k
    return T["k_odds_nar" if odds else "k_narrow"][ri], None


def reachable(P):
    """Every (kernel, reads per lane) some accepted call launches: fixed-length rows of every multiple of 16 up to the entry's
    limit, ragged rows up to the ragged pass' limit, two to four rows, with and without a cut, both arithmetics."""
    out = set()
    for odds in (False, True):
        for R in (2, 3, 4):
            out |= {dispatch(P, s, R, False, 0, odds) for s in range(16, P["max_stride"] + 1, 16)}
            out |= {dispatch(P, 640, R, True, split, odds) for split in (0, 7)}
    return out


def instance_key(inst):
    return kernel_of(inst), inst.k


# ---- the plan -------------------------------------------------------------------------------------------------------------------

def grid_blocks(nblk, cap=None):
    """Workgroups of the persistent grid (nar_grid_blocks; the library's own caps lie above what these batches ask for)."""
    blocks = (nblk + 3) // 4
    assert blocks <= MIN_CU_BLOCKS
    if cap:
        blocks = min(blocks, cap)
    return max(blocks, 1)


def walk(gw, nblk, W):
    """The blocks wave gw of W walks, in order."""
    return list(range(gw, nblk, W))


def seg_start(gw, nblk, W, per_blk):
    """Where wave gw's hand-back segment starts (the kernels' my_seg and k_nar_compact's src)."""
    return per_blk * (gw * (nblk // W) + min(gw, nblk % W))


def per_block(inst):
    return GROUP * (inst.k or 1)


def fixed_n(per_blk):
    return NBLK * per_blk - SHORT


def expected_waves(inst, n, grid):
    nblk = (n + per_block(inst) - 1) // per_block(inst)
    return 4 * grid_blocks(nblk, GRIDS[grid])


# ---- reads ----------------------------------------------------------------------------------------------------------------------

LAMBDA = {1: 0.001, 2: 0.023, 3: 0.19, 4: 0.48, 5: 0.85, 6: 8.0}      # expected errors per read for a target J (6: many rows)
AMB = ("", "", "", "", "", "", "N_first", "N_last", "N_border", "n")   # a role's ambiguous byte, drawn uniformly
J_BY_PATTERN = {"none": (1, 2), "all": (5, 6), "mixed": (1, 2, 3, 4, 5, 6)}


def _scores(rng, lens, target, stride):
    """One row per read: scores within a point of the one at which a read of its length has LAMBDA[target] expected errors."""
    lam = np.array([LAMBDA[int(t)] for t in target])
    qc = np.clip(np.rint(-10.0 * np.log10(np.minimum(lam / np.maximum(lens, 1), 0.7))), 2, 60).astype(np.int64)
    return (qc[:, None] + rng.integers(-1, 2, (len(lens), stride))).astype(np.uint8)


def _ambiguous(rng, q, lens, amb):
    for i in np.flatnonzero((np.asarray(amb) != "") & (lens > 0)):
        L = int(lens[i])
        if amb[i] == "N_first": q[i, 0] = 0
        elif amb[i] == "N_last": q[i, L - 1] = 0
        elif amb[i] == "N_border": q[i, max(0, (L - 1) // CHUNK * CHUNK - 1) if L > CHUNK else L - 1] = 0
        else: q[i, rng.integers(0, L)] = 255


def _padding(rng, q, lens):
    pad = np.arange(q.shape[1])[None, :] >= np.asarray(lens)[:, None]
    q[pad] = rng.integers(0, 256, int(pad.sum()), dtype=np.uint8)


def has_255(q, lens):
    return ((q == 255) & (np.arange(q.shape[1])[None, :] < np.asarray(lens)[:, None])).any(axis=1)


def border_pairs(patterns, W):
    return {(patterns[b], patterns[b + W]) for b in range(len(patterns) - W)}


WANTED_BORDERS = {("none", "all"), ("all", "none"), ("all", "all"), ("none", "none")}


def _positions(nblk, W):
    """block -> first / middle / last of its wave's walk (walks of one block: first)."""
    pos = {}
    for gw in range(min(W, nblk)):
        wk = walk(gw, nblk, W)
        for o, b in enumerate(wk):
            pos[b] = "first" if o == 0 else "last" if o == len(wk) - 1 else "middle"
    return pos


def block_patterns(rng):
    """A seeded draw of the 29 blocks' patterns, redrawn until both capped grids see every wanted border, a mixed block on each
    side of one, and a mixed block first, in the middle and last in a walk; the partial last block is mixed."""
    while True:
        p = [str(x) for x in rng.choice(["none", "all", "mixed"], NBLK)]
        p[NBLK - 1] = "mixed"
        ok = True
        for W in (4, 12):
            bp = border_pairs(p, W)
            pos = _positions(NBLK, W)
            ok &= WANTED_BORDERS <= bp and any(a == "mixed" for a, _ in bp) and any(b == "mixed" for _, b in bp)
            ok &= {pos[b] for b in range(NBLK) if p[b] == "mixed"} == {"first", "middle", "last"}
            r = NBLK % W                                        # the waves around the uneven border all hand reads back
            ok &= all(any(p[b] != "none" for b in walk(gw, NBLK, W)) for gw in (r - 1, r, r + 1))
        if ok:
            return p


class Batch:
    """q, lens (L everywhere for a fixed-length batch), and after refer(): the exact oracle's (ee, ns, pass), rows, the odds model."""

    def where(self):
        return dict(lens=self.lens) if self.ragged else dict(fixed_len=self.L)

    def refer(self, oracle):
        ex = oracle.filter_batch(self.q, threads=THREADS, **self.where())
        self.ex, self.rows = ex[:3], ex[3]
        self.m = oracle.filter_batch_model(self.q, "odds", threads=THREADS, **self.where())
        self.n255 = has_255(self.q, self.lens)
        return self

    def freeze(self):
        for a in (self.q, self.lens, self.rows, self.n255) + tuple(self.ex):
            a.setflags(write=False)
        return self

    def finished_odds(self, R):
        """F of tests/helpers/odds_forced.py: the reads a twin forced to R rows must finish itself."""
        return ~self.m.hand & ~self.n255 & (self.m.rows <= R)

    def handed(self, inst, rows_allowed=None):
        """Per read: does the instance hand it back?  rows_allowed: per read, for the mixed forms (ragged_groups)."""
        if inst.odds:
            return ~self.finished_odds(inst.R)
        R = inst.R if rows_allowed is None else rows_allowed
        return (self.rows > R) | self.n255 | np.isnan(self.ex[0])

    def crossing(self, inst):
        """(rows, reads whose row count is the whole story: no 'n', a result, and for a twin none the mode's guard hands back)."""
        if inst.odds:
            return self.m.rows, ~self.n255 & ~self.m.hand
        return self.rows, ~self.n255 & ~np.isnan(self.ex[0])


def _fixed_batch(oracle, L, stride, k):
    per_blk = GROUP * k
    n = fixed_n(per_blk)
    rng = np.random.default_rng([SEED, L, stride, k])
    b = Batch()
    b.L, b.stride, b.k, b.per_blk, b.n, b.ragged = L, stride, k, per_blk, n, False
    b.patterns = block_patterns(rng)
    blk = np.arange(n) // per_blk
    pat = np.array(b.patterns)[blk]
    target = np.zeros(n, np.int64)
    amb = np.array([""] * n, dtype=object)
    for name, js in J_BY_PATTERN.items():
        sel = np.flatnonzero(pat == name)
        target[sel] = rng.choice(js, len(sel))
        kinds = [a for a in AMB if (a != "n" or name != "none")] if name != "all" else ["", "", "n"]
        amb[sel] = rng.choice(np.array(kinds, dtype=object), len(sel))
    b.lens = np.full(n, L, np.int32)
    q = _scores(rng, b.lens, target, stride)
    _ambiguous(rng, q, b.lens, amb)
    _padding(rng, q, b.lens)
    b.q = q
    # what the roles aimed at and the oracle does not confirm is mended: in a `none` block a read that some instance would hand back
    # becomes a copy of one that none does; in an `all` block a read that some instance would finish gets an 'n'; the last read is
    # one every instance finishes (the lane pair (done, past the end))
    b.refer(oracle)
    any_back = (b.rows > 2) | b.n255 | np.isnan(b.ex[0]) | ~b.finished_odds(2)
    all_back = ((b.rows > 4) | b.n255 | np.isnan(b.ex[0])) & ~b.finished_odds(4)
    for blkno in range(NBLK):
        idx = np.flatnonzero(blk == blkno)
        if b.patterns[blkno] == "none":
            donors = idx[~any_back[idx]]
            for i in idx[any_back[idx]]:
                q[i] = q[donors[rng.integers(0, len(donors))]]
        elif b.patterns[blkno] == "all":
            for i in idx[~all_back[idx]]:
                q[i, rng.integers(0, L)] = 255
    if any_back[n - 1]:
        donors = np.flatnonzero(~any_back & (pat == "mixed"))
        q[n - 1] = q[donors[rng.integers(0, len(donors))]]
    return b.refer(oracle).freeze()


@functools.lru_cache(maxsize=None)
def fixed_batch(oracle, L, stride, k):
    """The shape's batch with its references: computed once, shared, never changed."""
    return _fixed_batch(oracle, L, stride, k)


# ---- the ledger of a fixed-length batch ------------------------------------------------------------------------------------------

def block_pattern(handed, b, per_blk, n):
    h = handed[b * per_blk:min(n, (b + 1) * per_blk)]
    return "none" if not h.any() else "all" if h.all() else "mixed"


def rows_that_exist(inst, L):
    """The crossing rows J = js + 1 the cells ask for: 1 .. R, and R + 1 (handed back by one row); a read of L bases has L + 1."""
    return [J for J in range(1, inst.R + 2) if J <= L + 1]


def pair_stores(inst):
    return inst.family == "rs" and inst.k == 2 and inst.R <= 3


PAIR_CELLS = [("pair", "done", "done"), ("pair", "done", "handed"), ("pair", "handed", "done"), ("pair", "handed", "handed"),
              ("pair", "done", "past")]


def required_fixed(inst, L):
    req = {("row", J, pos) for J in rows_that_exist(inst, L) for pos in ("first", "middle", "last")}
    req |= {("border",) + p for p in WANTED_BORDERS} | {("border", "mixed", "*"), ("border", "*", "mixed")}
    req |= {("uneven",), ("partial_last",)}
    if inst.family == "ring":
        req |= {("phase", 0)} | ({("phase", 1)} if ((L + 63) >> 6) % 2 else set())
    if pair_stores(inst):
        req |= set(PAIR_CELLS)
    return req


def fixed_ledger(inst, batch, grid):
    """The cells the batch fills for the instance on a grid: from the oracle's rows (the model's for a twin) and the plan."""
    per_blk, n = batch.per_blk, batch.n
    assert per_blk == per_block(inst)
    nblk = (n + per_blk - 1) // per_blk
    W = 4 * grid_blocks(nblk, GRIDS[grid])
    handed = batch.handed(inst)
    rows, plain = batch.crossing(inst)
    ncq = (batch.L + 63) >> 6
    cells = set()
    back = {}                                                 # wave -> reads it hands back
    for gw in range(min(W, nblk)):
        wk = walk(gw, nblk, W)
        back[gw] = sum(int(handed[b * per_blk:(b + 1) * per_blk].sum()) for b in wk)
        if len(wk) < 2:
            continue
        pats = [block_pattern(handed, b, per_blk, n) for b in wk]
        for o, b in enumerate(wk):
            pos = "first" if o == 0 else "last" if o == len(wk) - 1 else "middle"
            lo, hi = b * per_blk, min(n, (b + 1) * per_blk)
            for J in np.unique(rows[lo:hi][plain[lo:hi]]):
                cells.add(("row", int(J), pos))
            if inst.family == "ring":
                cells.add(("phase", (o * ncq) % 2))           # the ring slot the block's first panel lands in (two slots)
            if o >= 1:
                cells.add(("border", pats[o - 1], pats[o]))
                if pats[o - 1] == "mixed": cells.add(("border", "mixed", "*"))
                if pats[o] == "mixed": cells.add(("border", "*", "mixed"))
                if b == nblk - 1 and n % per_blk:
                    cells.add(("partial_last",))
                if pair_stores(inst):
                    for i0 in range(lo, hi, 2):
                        first = "handed" if handed[i0] else "done"
                        second = "past" if i0 + 1 >= n else "handed" if handed[i0 + 1] else "done"
                        cells.add(("pair", first, second))
    r = nblk % W
    if r >= 1 and r + 1 < min(W, nblk) and len(walk(r - 1, nblk, W)) == len(walk(r, nblk, W)) + 1 and min(back[r - 1], back[r], back[r + 1]) > 0:
        # wave r - 1 walks a block more than wave r; both and the next hand reads back, so that segment starts with and without the
        # min(gw, nblk % W) term are all read by k_nar_compact
        assert seg_start(r + 1, nblk, W, per_blk) - seg_start(r, nblk, W, per_blk) == per_blk * (nblk // W)
        assert seg_start(r, nblk, W, per_blk) - seg_start(r - 1, nblk, W, per_blk) == per_blk * (nblk // W + 1)
        cells.add(("uneven",))
    return cells


# ---- ragged batches --------------------------------------------------------------------------------------------------------------

def key_shift_of(stride, bins=64):
    ks = 0
    while ((stride >> 4) >> ks) >= bins:
        ks += 1
    return ks


def rag_order(lens, key_shift):
    """k_rag_sort: inside windows of 4096 consecutive reads, a stable sort by ceil(len / 16) >> key_shift -> the reads in walk order."""
    key = ((np.asarray(lens, np.int64) + 15) >> 4) >> key_shift
    return np.concatenate([w0 + np.argsort(key[w0:w0 + RG_WIN], kind="stable") for w0 in range(0, len(lens), RG_WIN)])


class Groups:
    """The groups of a ragged batch: order (reads in walk order), and per group maxc (16-byte chunks of its longest read), full
    (chunks complete in every read), panels, size."""

    def __init__(self, lens, key_shift):
        lens = np.asarray(lens, np.int64)
        self.order = rag_order(lens, key_shift)
        self.n, self.ngroups = len(lens), (len(lens) + GROUP - 1) // GROUP
        ln = lens[self.order]
        cuts = np.arange(0, self.n, GROUP)
        self.maxc = np.maximum.reduceat((ln + 15) >> 4, cuts)
        self.full = np.minimum.reduceat(ln >> 4, cuts)
        self.panels = np.maximum(1, (self.maxc + 7) >> 3)
        self.size = np.minimum(GROUP, self.n - cuts)
        self.group_of_read = np.empty(self.n, np.int64)
        self.group_of_read[self.order] = np.arange(self.n) // GROUP

    def reads(self, g):
        return self.order[g * GROUP:(g + 1) * GROUP]


def rows_allowed(inst, groups, split):
    """Per read: the rows its group runs with (mixed forms: RLO where the group's longest read has at most `split` chunks)."""
    per_group = np.where((inst.RLO < inst.R) & (groups.maxc <= split), inst.RLO, inst.R)
    return per_group[groups.group_of_read]


def _ragged_batch(oracle, lo, hi, stride):
    n = RAGGED_N
    rng = np.random.default_rng([SEED, lo, hi, stride])
    b = Batch()
    b.lo, b.hi, b.stride, b.n, b.ragged, b.L = lo, hi, stride, n, True, None
    b.key_shift = key_shift_of(stride)
    lens = rng.integers(lo, hi + 1, n).astype(np.int32)
    if lo == 0:
        lens[RG_WIN + rng.permutation(RG_WIN)[:100]] = 0       # one whole group of empty reads (they sort first in their window)
    b.lens = lens
    target = rng.choice(J_BY_PATTERN["mixed"], n)
    amb = rng.choice(np.array(AMB, dtype=object), n)
    q = _scores(rng, lens, target, stride)
    _ambiguous(rng, q, lens, amb)
    b.groups = G = Groups(lens, b.key_shift)
    b.planted = []
    for w in range(4):                                          # four pairs in each full window: groups 10 | 11, 24 | 25, ...
        for local in range(10, 10 + 14 * (PAIRS_PLANTED // 4), 14):
            g = w * (RG_WIN // GROUP) + local
            back, clean = G.reads(g), G.reads(g + 1)
            assert lens[back].min() >= 1
            q[back, 0] = 255
            q[clean] = rng.integers(58, 61, (GROUP, stride), dtype=np.uint8)
            b.planted.append(g)
    _padding(rng, q, lens)
    b.q = q
    return b.refer(oracle).freeze()


@functools.lru_cache(maxsize=None)
def ragged_batch(oracle, lo, hi, stride):
    return _ragged_batch(oracle, lo, hi, stride)


def required_ragged(inst, shape, grid):
    lo, hi, stride, split = shape
    req = {("window_border",)} if grid == "cap1" else set()
    if key_shift_of(stride) == 0:
        req |= {("straddle",), ("all_next_to_none",), ("partial_last_group",)}
        if lo == 0:
            req.add(("len0_group",))
        if inst.RLO < inst.R:
            req.add(("split_both",))
            if grid == "cap1":
                req.add(("rows_change",))
    return req


def ragged_ledger(inst, batch, shape, grid):
    """The cells the ragged batch fills.  Cells about two neighbouring groups count disjoint neighbouring pairs: W waves cut the walk
    W - 1 times, so W such pairs leave one inside a wave's range (the module's text)."""
    lo, hi, stride, split = shape
    G, n = batch.groups, batch.n
    W = 4 * grid_blocks(G.ngroups, GRIDS[grid])
    nwin = (n + RG_WIN - 1) // RG_WIN
    cells = set()
    if n == RAGGED_N and nwin == 5 and W == 4 and G.ngroups >= 10 * W:
        cells.add(("window_border",))                          # four interior borders, three cuts; tens of groups per wave
    if batch.key_shift:
        return cells
    allowed = rows_allowed(inst, G, split)
    handed = batch.handed(inst, allowed)
    per_group = np.add.reduceat(handed[G.order].astype(np.int64), np.arange(0, n, GROUP))

    def disjoint(hit):
        """How many disjoint pairs (g, g + 1) with hit[g]: a greedy count."""
        count, g = 0, 0
        while g < len(hit):
            if hit[g]:
                count, g = count + 1, g + 2
            else:
                g += 1
        return count

    if ((G.maxc == 0) & (G.size == GROUP)).any():
        cells.add(("len0_group",))
    ragged_end = G.full < G.maxc
    if disjoint((G.panels[:-1] != G.panels[1:]) & (ragged_end[:-1] | ragged_end[1:])) >= W:
        cells.add(("straddle",))
    whole, none = (per_group == G.size) & (G.size == GROUP), per_group == 0
    if disjoint((whole[:-1] & none[1:]) | (none[:-1] & whole[1:])) >= W:
        cells.add(("all_next_to_none",))
    if n % GROUP == 40 and G.size[-1] == 40:
        cells.add(("partial_last_group",))
    if inst.RLO < inst.R:
        short = G.maxc <= split
        per_win = RG_WIN // GROUP
        if all(short[w:w + per_win].any() and not short[w:w + per_win].all() for w in range(0, G.ngroups, per_win)):
            cells.add(("split_both",))
        if disjoint(short[:-1] != short[1:]) >= W:
            cells.add(("rows_change",))
    return cells
