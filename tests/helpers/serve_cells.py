"""Directed inputs for the resident per-read kernel (k_serve, moira_amd/csrc/mpb_kernels.hip): the cells of the register-resident
body of small_one_read<FMA = false, SYS = true>, of the gates it sits behind and of the thin bodies as k_serve really runs them, a
generator that fills them, and the ledger that says which were filled.  Plain Python and numpy; no GPU.

Which body answers a per-read call (li bases, p predicted rows, J rows needed = the oracle's `rows`):
  host    a score above 254 (a private code table) or li > 2047 (MPB_SERVE_STRIDE - 1): never posted to the kernel
  reg     li <= 1024 and p <= 64: one DP row per lane, ALL 64 rows looked at, so the read is finished whenever J <= 64 -- also when
          p < J (a thin body of cap < J would have missed it); J > 64: handed back (pass = 2), the host path answers
  sthin   otherwise, p <= 1024: the thin body of cap = max(2, next power of two >= p); J > cap: handed back
  wide    p > 1024: handed back at once
With MPB_SERVE=0 and in the broker's lanes form (k_small, a launch per call) there is no register body: every read of p <= 1024
runs the thin body of its cap.

p is the kernels' float sum in another order, so it is known only through the float64 statement of helpers/front_end_model.py and
its band, BAND = 0.01 + 1e-5 |x|.  A read is SURE when its thin cap is the same at both ends of the band (that settles every gate
above: p <= 64 <=> cap <= 64, p <= 1024 <=> cap <= 1024); the generator drops every other read, so no assertion leaves a read out.
Reads with an ambiguous base are the exception: under an 'n' marker (65536 in the float sum) a lane's sums step by 2^-7, under an
'N' marker (128) by 2^-16, which the band does not cover.  Such reads are kept only where the prediction cannot matter: at most
1024 bases, J <= 2 (every body looks at two rows) and at most 63 scored bases (rows <= scored + 1) or, without an 'n', a
prediction that stays <= 64 even one whole row beyond the band."""
import re

import numpy as np

from helpers import class_cells as CC
from helpers.device_runs import seq_and_quals
from helpers.front_end_model import BAND_ABS, BAND_REL, rows_of, x64

REG_MAX_BASES = 1024                      # the register body's gates: li <= 1024 && rows <= 64
REG_MAX_ROWS = 64
SERVE_STRIDE = 2048                       # MPB_SERVE_STRIDE: a mailbox row; reads of up to 2047 bases
CHUNK = 16                                # bytes a lane holds (yr); nchunks = (li + 15) >> 4
SMALL_MAX_STRIDE = 16384                  # MPB_SMALL_MAX_STRIDE: the lanes form runs longer reads alone
ALPHAS = CC.ALPHAS                        # (0.005, 0.05, 1e-6)
DEEP_ALPHAS = (1e-12, 1e-15)              # where a prediction falls short of J by whole rows, and J = 65 .. 67 with p <= 64
SEED = 20161019
PER_CELL = 2
MAX_READS = 1500
STRIDE = SERVE_STRIDE                     # of the packed matrices (holds the 2048-base read)


def parse_sources(kern, head):
    """The body's constants as mpb_kernels.hip and mpb_internal.h state them."""
    gate = re.search(r"if \(SYS && !FMA && li <= (\d+) && rows <= (\d+) && !\(prm\.flags & ~MPB_FLAG_ROUND\)\) \{", kern)
    nch = re.search(r"const int nchunks = \(li \+ (\d+)\) >> (\d+);", kern)
    walk = re.search(r"for \(int g = 0; g < (\d+) && js < 0; g\+\+\) \{", kern)
    define = lambda name: int(re.search(r"#define\s+%s\s+(\d+)\s" % name, head).group(1))
    return {"reg_max_bases": int(gate.group(1)), "reg_max_rows": int(gate.group(2)), "chunk": 1 << int(nch.group(2)),
            "chunk_round": int(nch.group(1)), "cdf_rows": int(walk.group(1)), "serve_stride": define("MPB_SERVE_STRIDE"),
            "small_max_stride": define("MPB_SMALL_MAX_STRIDE"), "tile_max_rows": define("MPB_TILE_MAX_ROWS")}


def tcap(p):
    """The thin body of a predicted row count: cap = max(2, next power of two >= p) (2048 and more: a wide read)."""
    p = np.maximum(np.asarray(p).astype(np.int64), 1)
    return np.maximum(2, 1 << np.ceil(np.log2(p)).astype(np.int64))


# ---- required cells --------------------------------------------------------------------------------------------------

JS_EDGE = (0, 1, 31, 32, 62, 63)
AMB = ("N_first", "N_last", "N_in_chunk63", "has_n", "only_N", "only_n", "len0")
GATES = ("li1024", "li1025", "rows64", "rows65", "rows128_short", "li2047", "li2048", "priv")
# ("reg", "under", k): J <= 64 in bin k and the thin cap of the prediction surely < J (a thin body would have missed the read);
# ("reg", "below", k): the prediction alone surely < J <= 64 (rows beyond the predicted budget are looked at)
UNDER_BINS = ((1, 7), (8, 15), (16, 31), (32, 48), (49, 64))


def required():
    """{cell: alphas at which it is required, or None (any alpha)}.  rows128_short is not in the list of gates a reader of the kernel
    would write down first: a read of li <= 1024 and 64 < p <= 128 that needs 64 < J <= 128 rows.  It is the only kind of read that
    tells `rows <= 64` from a wider gate (the register body would hand it back: one more solo read)."""
    req = {("reg", "js", j): (ALPHAS if j in JS_EDGE else ALPHAS[:1]) for j in range(REG_MAX_ROWS)}
    req.update({("reg", "chunks", c): None for c in (1, 2, 63, 64)})
    req.update({("reg", "tail", c, r): None for c in (1, 2, 64) for r in range(CHUNK)})
    req.update({("reg", "under", k): None for k in range(len(UNDER_BINS))})
    req.update({("reg", "below", k): None for k in range(len(UNDER_BINS))})
    req[("reg", "J65")] = None
    req.update({("reg", "amb", w): None for w in AMB})
    req.update({("gate", w): None for w in GATES})
    req.update({("sthin", c[1], c[2]): None for c in CC.thin_cells()})
    return req


GROUPS = ("js", "chunks", "tail", "under", "below", "J65", "amb", "gate", "sthin")


def group_of(cell):
    return cell[0] if cell[0] in ("gate", "sthin") else cell[1]


# the cells no input reaches, with the reason (test_serve_cells.py pins this list)
UNREACHABLE = {
    ("reg", "under", 4): "J in 49 .. 64 with a thin cap below J needs a prediction of at most 32 rows, 17 rows short; over 90,000 "
                         "two-quality reads of up to 1024 bases at alpha 1e-6 .. 1e-15 the prediction falls short by 7 rows at most "
                         "(the largest J with a thin cap below it: 36)",
}


# ---- the model of a batch ----------------------------------------------------------------------------------------------

class Pred:
    """Per read of a packed matrix: x (float64 predictor), scored, p_lo .. p_hi (rows at the ends of the band), cap_lo / cap_hi,
    amb (the read holds a byte 0 or 255), has_n, sure (see the module's text; J decides for the ambiguous ones: sure_with)."""

    def __init__(self, q, lens, alpha):
        q, lens = np.asarray(q), np.asarray(lens)
        xs, sc = [], []
        for at in range(0, len(lens), 2048):                          # (x64 makes float64 copies of the matrix)
            x, s = x64(q[at:at + 2048], lens[at:at + 2048], alpha)
            xs.append(x)
            sc.append(s)
        self.x = np.concatenate(xs) if xs else np.zeros(0)
        self.scored = np.concatenate(sc) if sc else np.zeros(0, np.int64)
        b = BAND_ABS + BAND_REL * np.abs(self.x)
        self.p_lo, self.p_hi = rows_of(self.x - b, self.scored), rows_of(self.x + b, self.scored)
        self.p_far = rows_of(self.x + b + 1.0, self.scored)
        self.cap_lo, self.cap_hi = tcap(self.p_lo), tcap(self.p_hi)
        live = np.arange(q.shape[1])[None, :] < lens[:, None]
        self.has_n = (live & (q == 255)).any(1)
        self.amb = self.has_n | (live & (q == 0)).any(1)
        self.lens = lens
        body = np.where(self.cap_hi > CC.TILE_MAX_ROWS, "wide", "sthin").astype(object)
        body[(lens <= REG_MAX_BASES) & ((self.cap_hi <= REG_MAX_ROWS) | self.amb)] = "reg"
        body[lens > SERVE_STRIDE - 1] = "host"
        self._body = body

    def sure_with(self, rows):
        """Plain reads: the thin cap is settled.  Ambiguous reads: the prediction cannot matter (rows = the oracle's J)."""
        J = np.asarray(rows)
        amb_ok = (self.lens <= REG_MAX_BASES) & (J <= 2) & ((self.scored + 1 <= REG_MAX_ROWS) | (~self.has_n & (self.p_far <= REG_MAX_ROWS)))
        return np.where(self.amb, amb_ok, self.cap_lo == self.cap_hi)

    def body(self):
        """"reg" / "sthin" / "wide" / "host" per read under k_serve (sure reads; an ambiguous sure read is a reg read)."""
        return self._body


def handed_back(pred, rows, nan, form):
    """Per sure read: does the kernel of a serving form hand it back (pass = 2 -> the broker runs it alone, `solo`)?
    form "serve": k_serve (the in-process entry, the broker's direct and copies forms); "lanes": k_small per micro-batch."""
    J = np.maximum(np.asarray(rows), 1)                               # no scored base: row 0 crosses (1.0 > 1 - alpha)
    miss_thin = ~pred.amb & ((J > pred.cap_hi) | (pred.cap_hi > CC.TILE_MAX_ROWS))
    if form == "lanes":
        return (pred.lens > SMALL_MAX_STRIDE - 1) | miss_thin | np.asarray(nan)
    body = pred.body()
    return (body == "host") | (body == "wide") | ((body == "reg") & (J > REG_MAX_ROWS)) | ((body == "sthin") & miss_thin) | np.asarray(nan)


# ---- the ledger ----------------------------------------------------------------------------------------------------------

def _under_bin(J):
    return [k for k, (lo, hi) in enumerate(UNDER_BINS) if lo <= J <= hi][0]


def cells_of_read(pred, i, row, J, nan, fine=False):
    """The cells one sure read fills (the pair gates li1024 / li1025 apart: ledger()).  fine: also the generator's own keys
    ("reg", "J65", J), which spread the reads it keeps."""
    li = int(pred.lens[i])
    out = set()
    if nan:
        return out
    body = pred.body()[i]
    if pred.amb[i]:
        live = np.asarray(row[:li])
        scored = ((live != 0) & (live != 255)).any()
        if live[0] == 0 and scored: out.add(("reg", "amb", "N_first"))
        if live[-1] == 0 and scored: out.add(("reg", "amb", "N_last"))
        if li > 63 * CHUNK and (live[63 * CHUNK:] == 0).any() and scored: out.add(("reg", "amb", "N_in_chunk63"))
        if (live == 255).any() and scored: out.add(("reg", "amb", "has_n"))
        if (live == 0).all(): out.add(("reg", "amb", "only_N"))
        if (live == 255).all(): out.add(("reg", "amb", "only_n"))
        return out
    if li == 0:
        return {("reg", "amb", "len0")}
    if li == SERVE_STRIDE:
        return {("gate", "li2048")}
    if body == "reg":
        c, r = (li + CHUNK - 1) // CHUNK, (li - 1) % CHUNK
        if 1 <= J <= REG_MAX_ROWS:
            out.add(("reg", "js", J - 1))
            if c in (1, 2, 63, 64): out.add(("reg", "chunks", c))
            if c in (1, 2, 64): out.add(("reg", "tail", c, r))
            if pred.cap_hi[i] < J: out.add(("reg", "under", _under_bin(J)))
            if pred.p_hi[i] < J: out.add(("reg", "below", _under_bin(J)))
            if pred.p_lo[i] == pred.p_hi[i] == REG_MAX_ROWS: out.add(("gate", "rows64"))
        elif J in (65, 66, 67):
            out.add(("reg", "J65"))
            if fine: out.add(("reg", "J65", J))
    elif body == "sthin":
        cap = int(pred.cap_hi[i])
        if 1 <= J <= cap and (li > REG_MAX_BASES or cap >= 128):
            out.add(("sthin", cap, J - 1))
            if li == SERVE_STRIDE - 1: out.add(("gate", "li2047"))
        if li <= REG_MAX_BASES and J <= 128:
            if pred.p_lo[i] == pred.p_hi[i] == REG_MAX_ROWS + 1: out.add(("gate", "rows65"))
            if pred.cap_hi[i] == 128 and J > REG_MAX_ROWS: out.add(("gate", "rows128_short"))
    return out


def ledger(batch, rows, nan):
    """{(cell, alpha)} a packed batch fills, from the oracle's rows and the model."""
    pred = batch.pred
    out = set()
    for i in range(batch.n):
        out |= {(c, batch.alpha) for c in cells_of_read(pred, i, batch.q[i], int(rows[i]), bool(nan[i]))}
    # the pair: the same 1024 bases, and with one Q60 base more that does not move J
    at1024 = {batch.q[i, :1024].tobytes(): i for i in np.nonzero(batch.lens == 1024)[0]}
    for k in np.nonzero((batch.lens == 1025) & (batch.q[:, 1024] == 60))[0]:
        i = at1024.get(batch.q[k, :1024].tobytes())
        if i is not None and rows[i] == rows[k] <= REG_MAX_ROWS and pred.body()[i] == "reg" and pred.body()[k] == "sthin" and rows[k] <= pred.cap_hi[k]:
            out |= {(("gate", "li1024"), batch.alpha), (("gate", "li1025"), batch.alpha)}
    return out


def ledger_all(oracle, batches):
    """{(cell, alpha)} of the whole set: every packed batch under the oracle's rows, and the PRIV reads."""
    filled = set()
    for b in batches:
        ee, _, _, rows = oracle_results(oracle, b)
        filled |= ledger(b, rows, np.isnan(ee))
    filled |= {(("gate", "priv"), a) for _, quals, a in PRIV if max(quals) > 254}
    return filled


def missing(filled, req=None):
    """The required cells that `filled` ({(cell, alpha)}) leaves empty, as (cell, alpha or None)."""
    req = required() if req is None else req
    out = []
    for cell, alphas in req.items():
        if cell in UNREACHABLE:
            continue
        if alphas is None:
            if not any(c == cell for c, _ in filled): out.append((cell, None))
        else:
            out += [(cell, a) for a in alphas if (cell, a) not in filled]
    return out


# ---- the generator ---------------------------------------------------------------------------------------------------------

class ServeBatch(CC.Batch):
    """The reads of one alpha as a packed matrix (stride 2048), with the model of their predictions."""

    def __init__(self, alpha, q, lens):
        CC.Batch.__init__(self, "serve_a%g" % alpha, "serve", alpha, q, lens)
        self.pred = Pred(q, self.lens, alpha)

    def triples(self):
        return [seq_and_quals(self.q[i], int(self.lens[i])) + (self.alpha,) for i in range(self.n)]


PER_READ = dict(ambigs="ignore", uncert=1.0)      # what a per-read call computes: Ns counted, never added; no limit


def oracle_results(oracle, batch, threads=8):
    """(ee, ns, pass, rows) of a packed batch as calculate_errors_PB defines them: one oracle call."""
    return oracle.filter_batch(batch.q, lens=batch.lens, alpha=batch.alpha, threads=threads, **PER_READ)


def _uniform(quals, lengths, stride):
    lens = np.tile(np.asarray(lengths, np.int32), len(quals))
    qv = np.repeat(np.asarray(quals, np.uint8), len(lengths))
    q = np.where(np.arange(stride)[None, :] < lens[:, None], qv[:, None], np.uint8(0)).astype(np.uint8)
    return q, lens


def _two(lows, ks, highs, lengths, stride):
    """k bases of a low quality, then a high one, L bases in all."""
    g = np.array([(lo, k, hi, L) for lo in lows for hi in highs for L in lengths for k in ks if k <= L], np.int64)
    col = np.arange(stride)[None, :]
    q = np.where(col < g[:, 1:2], g[:, 0:1], g[:, 2:3])
    q = np.where(col < g[:, 3:4], q, 0).astype(np.uint8)
    return q, g[:, 3].astype(np.int32)


def _pools():
    """[(name, alphas, (q, lens), oracle filter)]: the filter says which reads are worth the oracle's time, from the model."""
    reg_lens = sorted(set(range(1, 65)) | set(range(64, 1009, 5)) | set(range(1009, 1025)))
    reg_q = list(range(1, 46)) + [50, 60, 70]
    long_lens = sorted(set(range(1025, 2048, 6)) | {2047})
    big_j = sorted({c[2] + 1 for c in CC.thin_cells() if c[1] >= 128} | {65, 66})
    big_sel = lambda p: np.isin(p.p_hi, big_j + [j + 1 for j in big_j]) & (p.p_hi <= CC.TILE_MAX_ROWS)
    return [
        ("uniform1024", ALPHAS, _uniform(reg_q, reg_lens, 1024), lambda p: p.p_hi <= 70),
        ("two1024", DEEP_ALPHAS, _two((1, 2, 3), range(0, 61), (10, 15, 20, 30, 40), (60, 100, 200, 300, 500, 800, 1024), 1024),
         lambda p: p.p_hi <= 70),
        ("uniform2047", ALPHAS[:1], _uniform(list(range(8, 46)) + [50, 60, 70], long_lens, 2048), lambda p: p.p_hi <= 66),
        ("big2047", ALPHAS[:1], _uniform(range(1, 13), range(64, 2048, 3), 2048), big_sel),
        ("top2047", ALPHAS[:1], _uniform((1, 2, 3), range(1200, 2048), 2048), lambda p: p.p_hi == CC.TILE_MAX_ROWS),
    ]


def _specials():
    """Reads written down by hand, (name, row, alpha): the ambiguous ones (kept where the prediction cannot matter: Q45 and better,
    J <= 2), the mailbox limit, and the two sides of li <= 1024 (made from the kept 1024-base reads: _generate)."""
    def row(n, qv=45):
        return np.full(n, qv, np.uint8)
    out = []
    for a in ALPHAS[:2]:
        r = row(300); r[0] = 0; out.append(("N_first", r, a))
        r = row(300); r[-1] = 0; out.append(("N_last", r, a))
        r = row(37); r[-1] = 0; out.append(("N_last", r, a))
        r = row(1019); r[1010] = 0; out.append(("N_in_chunk63", r, a))
        r = row(1024); r[1023] = 0; out.append(("N_in_chunk63", r, a))
        r = row(40); r[5] = 255; out.append(("has_n", r, a))
        r = row(60); r[0] = 255; r[59] = 255; r[30] = 0; out.append(("has_n", r, a))
        out += [("only_N", row(1, 0), a), ("only_N", row(20, 0), a), ("only_n", row(20, 255), a), ("only_n", row(17, 255), a),
                ("len0", row(0), a)]
    out += [("li2047", row(2047, 30), ALPHAS[0]), ("li2048", row(2048, 30), ALPHAS[0]),
            ("li2047", np.where(np.arange(2047) % 2 == 0, 12, 14).astype(np.uint8), ALPHAS[1]),
            ("li2048", np.where(np.arange(2048) % 2 == 0, 12, 14).astype(np.uint8), ALPHAS[1])]
    return out


PRIV = [("ACGT" * 10, [300] * 40, 0.05), ("A" * 300, [30] * 299 + [255], 0.005)]       # a score above 254: its own code table


def _pad(rows):
    q = np.zeros((len(rows), STRIDE), np.uint8)
    for k, r in enumerate(rows):
        q[k, :len(r)] = r
    return q, np.array([len(r) for r in rows], np.int32)


def _generate(oracle):
    rng = np.random.default_rng(SEED)
    req = required()
    kept = {}                                                  # alpha -> [row bytes]
    have = {}                                                  # (cell, alpha) -> reads so far
    fine_keys = [("reg", "J65", j) for j in (65, 66, 67)]

    def wanted_at(alpha):
        total = lambda c: sum(v for (cc, _), v in have.items() if cc == c)
        w = {c for c, al in req.items() if (alpha in al if al is not None else total(c) < PER_CELL)}
        w |= {c for c in fine_keys if total(c) < PER_CELL}
        return w - {("reg", "J65")}                            # (asked for through its fine keys)

    def take(q, lens, alpha, sel_fn, per_cell):
        b = ServeBatch(alpha, q, lens)
        sel = np.ones(b.n, bool) if sel_fn is None else sel_fn(b.pred)
        idx = np.nonzero(sel)[0]
        rows, nan = np.full(b.n, -1, np.int32), np.ones(b.n, bool)
        if len(idx):
            ee, _, _, r = oracle.filter_batch(np.ascontiguousarray(q[idx]), lens=b.lens[idx], alpha=alpha, threads=CC._threads(oracle), **PER_READ)
            rows[idx], nan[idx] = r, np.isnan(ee)
        ok = sel & ~nan & b.pred.sure_with(rows)
        wanted = wanted_at(alpha)
        mine = {}
        cells = lambda i: {(c, alpha) for c in cells_of_read(b.pred, i, q[i], int(rows[i]), False, fine=True) if c in wanted}
        picked = CC._pick(np.nonzero(ok)[0], cells, {(c, alpha) for c in wanted}, per_cell, rng, mine)
        for k, v in mine.items():
            have[k] = have.get(k, 0) + v
        kept.setdefault(alpha, []).extend(q[i, :b.lens[i]].copy() for i in picked)
        return b, rows, ok

    for name, alphas, (q, lens), sel_fn in _pools():
        for alpha in alphas:
            b, rows, ok = take(q, lens, alpha, sel_fn, PER_CELL)
            if name == "uniform1024":
                # li <= 1024 from both sides: a kept-quality read of 1024 bases and the same with one Q60 base more, J unmoved
                cand = np.nonzero(ok & (b.lens == 1024) & (rows >= 1) & (rows <= REG_MAX_ROWS) & (b.pred.cap_hi <= REG_MAX_ROWS))[0]
                pair = np.zeros((2 * len(cand), 1040), np.uint8)
                pair[0::2, :1024] = q[cand]
                pair[1::2, :1024] = q[cand]
                pair[1::2, 1024] = 60
                pl = np.tile(np.array([1024, 1025], np.int32), len(cand))
                pb = ServeBatch(alpha, pair, pl)
                _, _, _, pr = oracle.filter_batch(pair, lens=pl, alpha=alpha, **PER_READ)
                good = [k for k in range(0, len(pl), 2) if pr[k] == pr[k + 1] and pb.pred.sure_with(pr)[k + 1]
                        and pb.pred.body()[k + 1] == "sthin" and pr[k + 1] <= pb.pred.cap_hi[k + 1]]
                for k in [good[j] for j in rng.permutation(len(good))[:PER_CELL]]:
                    kept[alpha] += [pair[k, :1024].copy(), pair[k + 1, :1025].copy()]
    by_alpha = {}
    for name, r, a in _specials():
        by_alpha.setdefault(a, []).append(r)
    for a, rows_ in by_alpha.items():
        q, lens = _pad(rows_)
        b = ServeBatch(a, q, lens)
        ee, _, _, r = oracle.filter_batch(q, lens=lens, alpha=a, **PER_READ)
        ok = ~np.isnan(ee) & b.pred.sure_with(r)
        kept.setdefault(a, []).extend(rows_[i] for i in np.nonzero(ok)[0])
    out = []
    for a in sorted(kept, reverse=True):
        uniq = {r.tobytes(): r for r in kept[a]}                  # a read kept for two cells is one read
        rows_ = [uniq[k] for k in sorted(uniq, key=lambda s: (len(s), s))]
        order = rng.permutation(len(rows_))
        q, lens = _pad([rows_[i] for i in order])
        out.append(ServeBatch(a, q, lens))
    return out


_CACHE = {}


def generate(oracle, fresh=False):
    """[ServeBatch], one per alpha (0.05, 0.005, 1e-6, 1e-12, 1e-15); PRIV holds the reads no packed row can state."""
    if fresh:
        return _generate(oracle)
    if "b" not in _CACHE:
        _CACHE["b"] = _generate(oracle)
    return _CACHE["b"]


def expected(oracle, batches):
    """{(batch index, read index): (ee, ns)} and {("priv", k): (ee, ns)}: one oracle call per alpha."""
    want = {}
    for bi, b in enumerate(batches):
        ee, ns, _, _ = oracle_results(oracle, b)
        want.update({(bi, i): (float(ee[i]), int(ns[i])) for i in range(b.n)})
    want.update({("priv", k): oracle.ee_rowwise(s, q, a)[:2] for k, (s, q, a) in enumerate(PRIV)})
    return want


def calls(batches):
    """[(key, seq, quals, alpha)] of every generated read, the PRIV reads last."""
    out = []
    for bi, b in enumerate(batches):
        out += [((bi, i),) + t for i, t in enumerate(b.triples())]
    return out + [(("priv", k), s, q, a) for k, (s, q, a) in enumerate(PRIV)]


def solo_expected(oracle, batches, form):
    """Reads the broker must run alone in a form ("serve": direct and copies; "lanes"): the PRIV reads and every read the form's
    kernel hands back (or never gets)."""
    n = len(PRIV)
    for b in batches:
        ee, _, _, rows = oracle_results(oracle, b)
        n += int(handed_back(b.pred, rows, np.isnan(ee), form).sum())
    return n


def sequences(oracle, batches):
    """{name: [call keys]}: orders in which to replay some of the reads.
      long_short         longest then shortest, three times over: stale bytes stay in the mailbox row and in the stage row behind the
                         short read's last chunk (2047 bases then 1 .. 17; 1024 then the same)
      sthin_reg_sthin    a thin-body read, a register-body read, a thin-body read ...: the wave's s_args and the light / fenced
                         completion alternate
      alphas             the three alphas call by call: the cached MpbDevParams on both sides change with every call"""
    by_len, sthin, reg = [], [], []
    for bi, b in enumerate(batches):
        body = b.pred.body()
        for i in range(b.n):
            by_len.append((int(b.lens[i]), bi, i))
            if body[i] == "sthin": sthin.append((bi, i))
            if body[i] == "reg" and not b.pred.amb[i] and b.lens[i] > 0: reg.append((bi, i))
    by_len.sort()
    served = [t for t in by_len if t[0] <= SERVE_STRIDE - 1]
    longest, regmax = served[-1], [t for t in served if t[0] <= REG_MAX_BASES][-1]
    short = [[t for t in served if t[0] == L][0] for L in (1, 2, 15, 16, 17) if any(t[0] == L for t in served)]
    seq = {"long_short": [], "sthin_reg_sthin": [], "alphas": []}
    for big in (longest, regmax):
        for s in short:
            seq["long_short"] += [big[1:], s[1:]]
    for k in range(12):
        seq["sthin_reg_sthin"] += [sthin[(7 * k) % len(sthin)], reg[(11 * k) % len(reg)]]
    seq["sthin_reg_sthin"].append(sthin[0])
    three = [bi for bi, b in enumerate(batches) if b.alpha in ALPHAS]
    for k in range(8):
        seq["alphas"] += [(bi, (5 * k + bi) % batches[bi].n) for bi in three]
    return seq
