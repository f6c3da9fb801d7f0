"""The sorted pipeline's front end -- k_prepass, k_classify_linear, k_scan, k_tables and the decode arithmetic -- stated in plain
float64 numpy, the band inside which its float sums may differ from that statement, and the batches that put the statement to
the test at the shapes where the kernels change path.  Plain Python and numpy; no GPU.

Row budget (class_read(), moira_amd/csrc/mpb_kernels.hip): over the scored bases of a read (bytes 1 .. 254 before its length)
    mu = sum p,  var = sum p (1 - p),  k3 = sum p (1 - p)(1 - 2 p),      p = 10^(-q / 10)
    x = mu + z sqrt(max(var, 1e-12)) + (k3 / max(var, 1e-12)) (z^2 - 1) / 6,      z = Phi^-1(1 - alpha)
    rows = floor(min(x, 1e9) + 0.5) + 1, halved under MPB_FLAG_TEST_UNDERPREDICT, clamped to 1 .. scored + 1
    budget = the smallest class cap >= rows, 0 (unreported) for a wide read (rows > 1024)
The kernels sum in float, in another order, with the hardware's exp2, so x is known only to within BAND = 0.01 + 1e-5 |x| (the
band test_gpu_no_crossing.py grants the float mu of the Chernoff test).  A read whose budget is the same at both ends of the
band is SURE: the library must report exactly that budget.  Any other read is UNSURE, and a batch may hold at most UNSURE_MAX of
them.  Neither figure follows what the kernels give: a sure read that disagrees is a finding."""
import numpy as np

from helpers.class_cells import CAPS, Batch, cap_of_rows, inv_norm_cdf

BAND_ABS, BAND_REL = 0.01, 1e-5
UNSURE_MAX = 0.05
ALPHAS = (0.005, 0.05, 1e-4)
SEED = 20161018

_P = 10.0 ** (-np.arange(256) / 10.0)
_P[0] = _P[255] = 0.0
_V = _P * (1.0 - _P)
_K = _V * (1.0 - 2.0 * _P)


def x64(q, lens, alpha):
    """(x, scored) of every read of a packed matrix: class_read()'s predictor in float64, and the count of scored bases."""
    q, lens = np.asarray(q), np.asarray(lens)
    code = np.where(np.arange(q.shape[1])[None, :] < lens[:, None], q, np.uint8(0))
    mu, var, k3 = _P[code].sum(1), _V[code].sum(1), _K[code].sum(1)
    scored = ((code != 0) & (code != 255)).sum(1)
    z = inv_norm_cdf(1 - alpha)
    v = np.maximum(var, 1e-12)
    return mu + z * np.sqrt(v) + (k3 / v) * ((z * z - 1) / 6), scored


def rows_of(x, scored, underpredict=False):
    rows = np.floor(np.minimum(x, 1e9) + 0.5).astype(np.int64) + 1
    if underpredict:
        rows = rows // 2
    return np.maximum(np.minimum(rows, scored + 1), 1)


class Model:
    """Per read: x, scored, rows (at x), sure, and budget -- the cap a sure read must be given (0: wide), -1 for an unsure one,
    whose budget is only bracketed by lo .. hi (caps, or 0)."""

    def __init__(self, q, lens, alpha, underpredict=False):
        self.x, self.scored = x64(q, lens, alpha)
        b = BAND_ABS + BAND_REL * np.abs(self.x)
        self.rows = rows_of(self.x, self.scored, underpredict)
        self.lo = cap_of_rows(rows_of(self.x - b, self.scored, underpredict))
        self.hi = cap_of_rows(rows_of(self.x + b, self.scored, underpredict))
        self.sure = self.lo == self.hi
        self.budget = np.where(self.sure, self.lo, -1).astype(np.int32)
        self.unsure_share = float((~self.sure).mean()) if len(self.sure) else 0.0


def overflow_bracket(model, oracle_rows, among=None):
    """(A, A + U) of assertion (d): A = sure tile reads whose oracle rows exceed their budget, U = unsure reads and the reads of
    model budget 0 (a wide read's own budget is reported by no entry).  among: a mask that restricts the count."""
    m = np.ones(len(model.sure), bool) if among is None else np.asarray(among)
    tile = model.sure & (model.budget > 0) & m
    a = int((tile & (np.asarray(oracle_rows) > model.budget)).sum())
    return a, a + int((m & ~tile).sum())


# ---- the input families ----------------------------------------------------------------------------------------------

# name: (row stride, shortest and longest read, lowest and highest base quality `lo` of a read)
FAMILIES = {"good": (320, 20, 300, 25, 40), "mixed": (960, 1, 960, 2, 40), "mid976": (976, 1, 976, 5, 29),
            "short16": (16, 0, 16, 1, 40), "bad": (2048, 900, 2048, 1, 7), "wide": (4096, 1400, 4096, 1, 2)}


def family_q(rng, n, stride, lo_lo, lo_hi, ambiguous=True):
    """n rows of `stride` bytes: per read a base quality lo, bytes uniform in [lo, min(42, lo + 8)), 1 % byte 0 and 0.3 % byte 255.
    Every byte of the row is drawn: what lies past a read's length is not zeroed (the kernels mask it)."""
    lo = rng.integers(lo_lo, lo_hi + 1, n)
    width = np.minimum(42, lo + 8) - lo
    q = (lo[:, None] + (rng.random((n, stride), np.float32) * width[:, None]).astype(np.int64)).astype(np.uint8)
    if ambiguous:
        r = rng.random((n, stride), np.float32)
        q[r < 0.01] = 0
        q[(r >= 0.01) & (r < 0.013)] = 255
    return q


def family_batch(name, n, alpha, seed=0):
    """n reads of a family at its own stride, ragged (the CPU measurement of the unsure share)."""
    stride, l0, l1, q0, q1 = FAMILIES[name]
    rng = np.random.default_rng(SEED + seed)
    return Batch("%s_%d" % (name, n), name, alpha, family_q(rng, n, stride, q0, q1), rng.integers(l0, l1 + 1, n))


def group_lens(rng, n, stride):
    """Ragged lengths for the 16-read groups of k_prepass: inside every group one read of no bases, one of the full stride, one
    each of 16 k - 1 / 16 k / 16 k + 1 for a random k, the rest random; group 1 has sixteen equal lengths.  (The last group
    straddles n whenever n % 16 != 0.)"""
    lens = rng.integers(0, stride + 1, n)
    for g0 in range(0, n, 16):
        k = int(rng.integers(1, max(2, stride // 16)))            # 16 k + 1 fits the row (stride 16: it is cut to 16)
        special = [0, stride, 16 * k - 1, 16 * k, min(stride, 16 * k + 1)]
        at = g0 + rng.permutation(16)[:5]
        for i, v in zip(at, special):
            if i < n:
                lens[i] = v
    if n >= 32:
        lens[16:32] = int(rng.integers(1, stride + 1))
    return lens.astype(np.int32)


N_SWEEP = (1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049)        # lane group, wave, round, block
SCAN_N = (262144, 262145)                                                            # 256 and 257 blocks: k_scan's seg 1 -> 2
SWEEP_N = 1100                                                                       # a block, a wave and 12 reads
SWEEP = {16: "short16", 64: "mixed", 320: "good", 944: "mixed", 960: "mixed", 976: "mid976", 1024: "mid976", 1936: "bad",
         2048: "bad", 4096: "wide"}                                                  # stride: the family that fits
FIXED_CUTS = (0, 1, 15, 16)                                                          # fixed lengths stride - cut
FIXED_ALPHAS = (0.05, 1e-4, 0.05, 0.005)                                             # ... and the alpha of each
MARKER_STRIDES = (960, 976, 1920, 1936)
# strides at which k_classify_linear's geometry changes: (tile_rows, lanes per row)
LINEAR_GEOMETRY = {32: (640, 1), 48: (426, 1), 80: (256, 1), 1264: (16, 16), 1280: (16, 16), 1296: (15, 16), 10240: (2, 64),
                   10256: (1, 64), 16384: (1, 64)}
LISTED_M = (1, 63, 64, 65, 1023, 1025)
LISTED_N, LISTED_STRIDE, LISTED_FIXED = 4096, 320, 300

_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def linear_geometry(stride):
    """(tile_rows, lanes per row) of k_classify_linear at a row stride, as the kernel derives them."""
    cpr = stride // 16
    tile_rows = max(1, min(1024, 1280 // cpr))
    lpr = 1
    while lpr < 64 and lpr * 2 * tile_rows <= 256:
        lpr *= 2
    return tile_rows, lpr


def _alpha(k):
    return ALPHAS[k % len(ALPHAS)]


def n_sweep_batch(n, ragged):
    """Stride 48, the `mixed` qualities: fixed length 40, or ragged 0 .. 48."""
    def make():
        rng = np.random.default_rng(SEED + 100 + n)
        q = family_q(rng, n, 48, 2, 40)
        lens = rng.integers(0, 49, n) if ragged else np.full(n, 40)
        return Batch("n%d_%s" % (n, "ragged" if ragged else "fixed40"), "mixed", _alpha(N_SWEEP.index(n)), q, lens,
                     fixed_len=None if ragged else 40)
    return _cached(("n", n, ragged), make)


def scan_batch(n, ragged):
    """Stride 32: fixed length 32, or ragged 0 .. 32.  The 262,144 reads are the first rows of the 262,145."""
    def make():
        rng = np.random.default_rng(SEED + 200 + ragged)
        top = max(SCAN_N)
        return family_q(rng, top, 32, 2, 40), (rng.integers(0, 33, top) if ragged else np.full(top, 32))
    q, lens = _cached(("scan", ragged), make)
    return Batch("scan%d_%s" % (n, "ragged" if ragged else "fixed32"), "mixed", 0.005, q[:n], lens[:n], fixed_len=None if ragged else 32)


def sweep_batch(stride, cut=None, n=None):
    """The stride sweep: cut None = ragged (group_lens), else the fixed length stride - cut, on the same bytes."""
    fam = SWEEP.get(stride) or ("short16" if stride < 64 else "mixed")
    n = n or SWEEP_N

    def make():
        rng = np.random.default_rng(SEED + 300 + stride)
        _, _, _, q0, q1 = FAMILIES[fam]
        return family_q(rng, n, stride, q0, q1), group_lens(rng, n, stride)
    q, lens = _cached(("sweep", stride, n), make)
    k = stride // 16
    if cut is None:
        return Batch("s%d_ragged" % stride, fam, _alpha(k), q, lens)
    return Batch("s%d_fixed%d" % (stride, stride - cut), fam, FIXED_ALPHAS[FIXED_CUTS.index(cut)], q, np.full(n, stride - cut),
                 fixed_len=stride - cut)


def linear_batch(stride, ragged):
    """The strides of LINEAR_GEOMETRY.  Below 10240: the sweep's shape with n = max(1100, 2 tile_rows + 3), so that a block walks
    whole tiles and a partial one.  From 10240 on: 40 good and middling reads (lo >= 20) and one wide read (Q1 throughout)."""
    if stride < 10240:
        n = max(SWEEP_N, 2 * linear_geometry(stride)[0] + 3)
        return sweep_batch(stride, None if ragged else 0, n)

    def make():
        rng = np.random.default_rng(SEED + 400 + stride)
        q = family_q(rng, 40, stride, 20, 40)
        q[7, :] = 1
        lens = group_lens(rng, 40, stride)
        lens[7] = stride
        return q, lens
    q, lens = _cached(("linear", stride), make)
    if ragged:
        return Batch("s%d_ragged" % stride, "good", 0.005, q, lens)
    return Batch("s%d_fixed%d" % (stride, stride), "good", 0.05, q, np.full(40, stride), fixed_len=stride)


MARKER_KINDS = ("all_N", "all_n", "N_n_alternating", "N_then_n", "scored_last_chunk_N", "scored_last_chunk_n", "scored_first_n",
                "scored_last_n")


def marker_batch(stride):
    """Rows of ambiguity markers (k_prepass peels their counts off a float sum, per panel of 960 bytes): every kind of
    MARKER_KINDS at the lengths stride, stride - 1, stride - 16, 961, 960 and 481, among reads of the `mixed` family."""
    def make():
        rng = np.random.default_rng(SEED + 500 + stride)
        lengths = [L for L in (stride, stride - 1, stride - 16, 961, 960, 481) if L <= stride]
        n = 16 * ((len(MARKER_KINDS) * len(lengths) + 16 + 15) // 16) + 5
        q = family_q(rng, n, stride, 2, 40)
        lens = rng.integers(1, stride + 1, n).astype(np.int32)
        rows = rng.permutation(n)[:len(MARKER_KINDS) * len(lengths)]
        col = np.arange(stride)
        kinds = []
        for j, i in enumerate(rows):
            kind, L = MARKER_KINDS[j % len(MARKER_KINDS)], lengths[j // len(MARKER_KINDS)]
            score = q[i].copy()
            score[(score == 0) | (score == 255)] = 3
            last16 = (col >= 16 * ((L - 1) // 16)) & (col < L)
            q[i] = {"all_N": 0, "all_n": 255, "N_n_alternating": np.where(col % 2 == 0, 0, 255),
                    "N_then_n": np.where(col < L // 2, 0, 255), "scored_last_chunk_N": np.where(last16, score, 0),
                    "scored_last_chunk_n": np.where(last16, score, 255), "scored_first_n": np.where(col == 0, score, 255),
                    "scored_last_n": np.where(col == L - 1, score, 255)}[kind]
            lens[i] = L
            kinds.append((int(i), kind, L))
        return q, lens, kinds
    q, lens, kinds = _cached(("marker", stride), make)
    b = Batch("markers%d" % stride, "mixed", 0.005, q, lens)
    b.kinds = kinds
    return b


def listed_batch(oracle, m, ragged):
    """4,096 good reads (lo >= 35, no 'n'; one that would need more than two rows at alpha 0.005, or whose budget the band leaves
    open -- at a fixed length the reads of one lo lie in one cluster of x, which may sit on a class edge -- is replaced by Q41 throughout)
    at stride 320, fixed length 300 or ragged 20 .. 300, with exactly m reads planted that a two-row narrow pass must hand back:
    half of them reads of the `bad` family (lo 1 .. 7, at least 100 bases), half good reads with one byte 255; at scattered
    indices that include 0 and n - 1.  -> (Batch, planted indices, oracle result)."""
    def make():
        rng = np.random.default_rng(SEED + 600 + 2 * m + ragged)
        n, stride = LISTED_N, LISTED_STRIDE
        q = family_q(rng, n, stride, 35, 40, ambiguous=False)
        q[rng.random((n, stride)) < 0.002] = 0
        lens = (rng.integers(20, 301, n) if ragged else np.full(n, LISTED_FIXED)).astype(np.int32)
        rows = oracle.filter_batch(q, lens=lens, alpha=0.005, threads=8)[3]
        q[(rows > 2) | ~Model(q, lens, 0.005).sure] = 41          # (Q41 throughout: two rows, and sure at every length here)
        # the planted good reads come from those the model is sure of (they lie in a few clusters of x, one of which may sit on
        # a class edge): the band may hide at most 5 % of what is handed back
        sure = np.flatnonzero(Model(q, lens, 0.005).sure[1:n - 1]) + 1
        n_bad, n_low = (m + 1) // 2, m // 2
        low = np.r_[n - 1, rng.permutation(sure)[:n_low - 1]] if n_low else np.zeros(0, np.int64)
        rest = np.setdiff1d(np.arange(1, n - 1), low)
        bad_at = np.r_[0, rng.permutation(rest)[:n_bad - 1]]
        bad = family_q(rng, n_bad, stride, 1, 7)
        for j, i in enumerate(bad_at):
            q[i] = bad[j]
            lens[i] = max(int(lens[i]), 100)
        for i in low:
            q[i, int(rng.integers(0, lens[i]))] = 255
        at = np.sort(np.r_[bad_at, low]).astype(np.int64)
        b = Batch("listed%d_%s" % (m, "ragged" if ragged else "fixed"), "good", 0.005, q, lens, fixed_len=None if ragged else LISTED_FIXED)
        return b, at, oracle.filter_batch(q, lens=lens, alpha=0.005, threads=8)
    return _cached(("listed", m, ragged), make)


def front_end_batches():
    """Every batch the GPU tests of k_prepass / k_classify_linear run (the LISTED ones apart: they need the oracle)."""
    out = [n_sweep_batch(n, r) for n in N_SWEEP for r in (False, True)]
    out += [scan_batch(n, r) for n in SCAN_N for r in (False, True)]
    out += [sweep_batch(s, c) for s in SWEEP for c in (None,) + FIXED_CUTS]
    out += [marker_batch(s) for s in MARKER_STRIDES]
    out += [linear_batch(s, r) for s in LINEAR_GEOMETRY for r in (True, False)]
    return out


# ---- the decode bytes --------------------------------------------------------------------------------------------------

DECODE_N, DECODE_STRIDE = 512, 272
SWAR_OFFSETS = (1, 33, 64, 127, 128, 129, 255)          # decode4: word-wide arithmetic
BYTE_OFFSETS = (0, -5, 256, 300)                        # decode4_bytes throughout
N_NEIGHBOURS = (0x4F, 0x6F, 0x0E, 0x2E, 0xCE, 0xEE, 0x4C, 0x6C, 0x4A, 0x6A, 0x46, 0x66, 0x5E, 0x7E)   # one bit from 'N' / 'n'


def decode_inputs():
    """(seq, qual, ragged lens): 512 x 272 letter and quality bytes in which every quality byte meets every letter byte -- the
    65,536 pairs, shuffled, fill the first 241 rows; the other rows hold random pairs in which half the letters are 'N', 'n' or
    one bit away from them -- and ragged lengths 0 .. 272 that take every residue mod 16 (all pairs are live at fixed length 272)."""
    def make():
        rng = np.random.default_rng(SEED + 700)
        n, stride = DECODE_N, DECODE_STRIDE
        pairs = rng.permutation(65536)
        cells = np.r_[pairs, rng.integers(0, 65536, n * stride - 65536)]
        seq, qual = (cells >> 8).astype(np.uint8), (cells & 255).astype(np.uint8)
        near = np.frombuffer(bytes(N_NEIGHBOURS) + b"NnNnNnACGT", np.uint8)
        tail = np.arange(n * stride) >= 65536
        swap = tail & (rng.random(n * stride) < 0.5)
        seq[swap] = rng.choice(near, int(swap.sum()))
        seq, qual = seq.reshape(n, stride), qual.reshape(n, stride)
        lens = (stride - (np.arange(n) * 7) % (stride + 1)).astype(np.int32)
        lens[-3:] = (0, 1, stride)
        lens[:241] = stride - np.arange(241) % 17                    # the rows that hold the 65,536 pairs stay nearly whole
        return seq, qual, lens
    return _cached("decode", make)


def decode_rule(seq, qual, lens, offset):
    """(packed matrix, count of undecodable bytes): decode4_bytes in numpy."""
    live = np.arange(seq.shape[1])[None, :] < np.asarray(lens)[:, None]
    qv = qual.astype(np.int64) - offset
    bad = live & ((qv < 0) | (qv > 254))
    out = np.where(qv < 0, 1, np.where(qv > 254, 254, np.where(qv == 0, 1, qv)))
    out = np.where(seq == ord("N"), 0, np.where(seq == ord("n"), 255, out))
    return np.where(live, out, 0).astype(np.uint8), int(bad.sum())
