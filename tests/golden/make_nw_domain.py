#!/usr/bin/env python3
"""Generate tests/golden/nw_domain.npz from the REAL reference: the edges of what the paired-contig path accepts.

Run where make_golden.py runs (it needs the reference checkout that make_golden.REF names):
    python tests/golden/make_nw_domain.py

As make_golden.py does for nw_pairs.npz: moira/nw_align.pyx is cythonized and compiled in a temp dir outside the repo,
moira.py is loaded through make_golden.load_python_reference, both are used and deleted.  Only data is written: the inputs and
what the reference made of them (its aligned strings as one move per alignment column -- 0 both reads, 1 the forward read alone,
2 the mate alone; no read holds a '-', so the strings follow from the reads and the moves --, its score, and make_contig's
contig, qualities and overlap / gaps / mismatches).  Every case is one pair with qualities and every parameter; `part` says
why it is there:

  0  alignments   17 scoring sets (near the 16-bit boundary, zero and negative, sign-reversed and positive, gap- and
                  mismatch-dominated), per set the largest l1 = l2 the predicate (l1 + l2 + 2) * max|param| < 30000 allows and
                  l1, l2 at the C boundaries 1, 64, 65, 128, 129, 256, 257, 384 where it allows them; the five kinds of
                  contig_pairs.make_pair in rotation
  1  predicate    four values of max|param|, one pair with (l1 + l2 + 2) * max|param| in 29,900..29,999 (built) and one with
                  it in 30,000..30,100 (handed back; the host takes its 32-bit walk)
  2  fix-up       short tie-heavy pairs found by search, so that every outcome of the 3' fix-up occurs (`fixup`, bit per class:
                  1 nothing to rewrite, 2 the column wins strictly, 4 the row wins strictly, 8 equal maxima (the row is
                  rewritten), 16 the winning column holds its maximum twice, 32 the winning row holds its maximum twice)
  3  contigs      offsets 33 / 64 / 0 with qualities 0..93 / 0..62 / 0..119, best / sum / posterior, caps 0 / 40 / 93, trim,
                  (insert, deltaq) of (1, 1), (20, 6), (60, 50), bases from ACGTNWSRYMKBVDH with 15 % non-ACGT, default scoring
                  for two thirds and the scoring sets in rotation for the rest
  4  hot          a few contig pairs whose qualities lie ABOVE those ranges: inside them the largest contig quality byte is
                  242 (offset 0: posterior of 119 and 119), so no contig quality can leave its byte; eight pairs make it happen, and
                  two more end exactly ON the byte (127 + 128 at offset 0: built, and refused by the text filter)

Parts 0-2 carry qualities 2..41 from a fixed formula (no random stream) at offset 33 and the default consensus setting.
`built` is what the device must do with the case: 1 when the predicate holds and every contig quality q of the reference has
0 <= q and q + offset <= 255, else 0; `cause` says why not (1 predicate, 2 a quality above the byte, 3 a quality below zero).
The fix-up class of every case comes from a plain numpy restatement of the fill (restate() below), whose alignment and score
must be the Cython aligner's for every pair.  The conditions at the end of main() are asserted before anything is written.
The archive is written with fixed timestamps: a second run gives the same bytes.
"""
import io
import os
import shutil
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [HERE, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "helpers"), ROOT]
import make_golden as MG          # noqa: E402
import contig_pairs as P          # noqa: E402

SCORING = [(39, -39, -39), (77, -76, -75), (100, -99, -100), (7499, -7499, -7499),           # near the 16-bit boundary
           (0, 0, 0), (-1, -1, -1), (-3, -2, -1), (0, -1, -1), (0, 0, -1),                   # zero and negative
           (1, -1, 1), (-2, 3, -1), (0, 5, 0), (3, 2, 1), (1, 1, 1),                         # sign-reversed and positive
           (1, -1, 0), (2, -3, -1000), (1, -29, -2)]                                          # gap- / mismatch-dominated
DEFAULT = (1, -1, -2)
PREDICATE_ROWS = [(39, -39, -39), (77, -76, -75), (100, -99, -100), (111, -110, -111)]
BOUND = (1, 64, 65, 128, 129, 256, 257, 384)
KINDS = ("overlap", "ties", "unrelated", "contained", "identical")
MODES = ("best", "sum", "posterior")
IUPAC = "NWSRYMKBVDH"
N_CONTIGS = 850
SIZE_LIMIT = 500000


def maxabs(prm):
    return max(abs(v) for v in prm)


def predicate(l1, l2, prm):
    return (l1 + l2 + 2) * maxabs(prm) < 30000


def fixed_quals(n, salt):
    return [2 + (7 * k + salt) % 40 for k in range(n)]


def restate(x, y, match, mismatch, gap):
    """moira/nw_align.pyx restated: the fill by anti-diagonals, the 3' fix-up, the traceback that sums the path's cells
    -> (aln1, aln2, score, fixup class bits)."""
    n1, n2 = len(x), len(y)
    a, b = np.frombuffer(x.encode(), np.uint8), np.frombuffer(y.encode(), np.uint8)
    sub = np.where(a[:, None] == b[None, :], match, mismatch).astype(np.int64)
    S = np.zeros((n1 + 1, n2 + 1), np.int64)
    D = np.zeros((n1 + 1, n2 + 1), np.int8)              # 0 diagonal, 1 up, 2 left
    D[:, 0] = 1
    D[0, 1:] = 2
    for d in range(2, n1 + n2 + 1):
        i = np.arange(max(1, d - n2), min(n1, d - 1) + 1)
        j = d - i
        dg, up, lf = S[i - 1, j - 1] + sub[i - 1, j - 1], S[i - 1, j] + gap, S[i, j - 1] + gap
        take_d = (dg >= up) & (dg >= lf)
        take_u = ~(dg >= up) & (up >= lf)
        S[i, j] = np.where(take_d, dg, np.where(take_u, up, lf))
        D[i, j] = np.where(take_d, 0, np.where(take_u, 1, 2))
    col, row = S[:, n2], S[n1, :]
    cs, rs = int(col.max()), int(row.max())
    bci, bri = int(np.nonzero(col == cs)[0][-1]), int(np.nonzero(row == rs)[0][-1])      # the LAST >= maximum
    if bci == n1 and bri == n2:
        cls = 1
    elif cs > rs:
        D[bci + 1:, n2] = 1
        cls = 2 | (16 if int((col == cs).sum()) >= 2 else 0)
    else:
        D[n1, bri + 1:] = 2
        cls = (4 if rs > cs else 8) | (32 if int((row == rs).sum()) >= 2 else 0)
    i, j, score, o1, o2 = n1, n2, 0, [], []
    while i > 0 or j > 0:
        score += int(S[i, j])
        mv = int(D[i, j])
        o1.append(x[i - 1] if mv != 2 else "-")
        o2.append(y[j - 1] if mv != 1 else "-")
        i -= mv != 2
        j -= mv != 1
    return "".join(reversed(o1)), "".join(reversed(o2)), score, cls


def moves_of(a1, a2):
    return np.array([0 if (c != "-" and d != "-") else (1 if c != "-" else 2) for c, d in zip(a1, a2)], np.uint8)


def overlap_window(a1, a2):
    f = [k for k, c in enumerate(a1) if c != "-"]
    r = [k for k, c in enumerate(a2) if c != "-"]
    return (r[0], f[-1]) if f[0] < r[0] else (f[0], r[-1])


def with_iupac(rng, s, share=0.15):
    s = list(s)
    for pos in np.nonzero(rng.random(len(s)) < share)[0]:
        s[pos] = IUPAC[int(rng.integers(0, len(IUPAC)))]
    return "".join(s)


def run_quals(rng, n, qmax):
    """Qualities 0..qmax in runs of 1..8 equal values (as real reads have them, and the archive stays small); a pair in five
    has typical qualities (2..41) instead, one in ten holds zeros and the top value."""
    style = int(rng.integers(0, 10))
    out = []
    while len(out) < n:
        if style < 2:
            v = int(rng.integers(2, min(41, qmax) + 1))
        elif style == 2:
            v = int(rng.choice([0, 0, 1, qmax, qmax - 1, int(rng.integers(0, qmax + 1))]))
        else:
            v = int(rng.integers(0, qmax + 1))
        out += [v] * int(rng.integers(1, 9))
    return out[:n]


class Cases:
    def __init__(self, nw, pyref):
        self.nw, self.pyref, self.rows = nw, pyref, []

    def add(self, part, fwd, mate, q1, q2, prm, mode="best", cap=40, trim=False, insert=20, deltaq=6, offset=33):
        """q2 runs along the mate as it aligns.  The mate goes through the reference's reverse_complement from the record the
        FASTQ file would hold (and back), the pair through its aligner and its make_contig."""
        assert 1 <= len(fwd) <= 384 and 1 <= len(mate) <= 384 and not set(fwd + mate) & set(".-")
        record, record_q = self.pyref.reverse_complement(mate, list(q2))
        back, back_q = self.pyref.reverse_complement(record, list(record_q))
        assert (back, back_q) == (mate, list(q2)) and record == P.revcomp(mate)
        a1, a2, score = self.nw.nw_align(fwd, mate, prm[0], prm[1], prm[2])
        r1, r2, rscore, cls = restate(fwd, mate, *prm)
        assert (r1, r2, rscore) == (a1, a2, score), (fwd, mate, prm)
        raised = 0
        try:
            contig, cq, ov, gaps, mism = self.pyref.make_contig(a1, list(q1), a2, list(q2), insert, deltaq, mode, cap, trim)
            cq = [int(v) for v in cq]
        except Exception:                                # recorded, not hidden: the host must raise as well
            raised, contig, cq, ov, gaps, mism = 1, "", [], 0, 0, 0
        cause = 0
        if not predicate(len(fwd), len(mate), prm):
            cause = 1
        elif raised:
            cause = 4
        elif any(q + offset > 255 for q in cq):
            cause = 2
        elif any(q < 0 for q in cq):
            cause = 3
        hot = 0                                          # posterior look-ups with a quality above 41
        if mode == "posterior" and not raised:
            lo, hi = overlap_window(a1, a2)
            qa, qb, u, v = [], [], 0, 0
            for c, d in zip(a1, a2):
                qa.append(q1[u] if c != "-" else -1); u += c != "-"
                qb.append(q2[v] if d != "-" else -1); v += d != "-"
            hot = sum(1 for k in range(lo, hi + 1) if qa[k] >= 0 and qb[k] >= 0 and max(qa[k], qb[k]) > 41 and
                      (a1[k] == a2[k] or qa[k] != qb[k]))
        self.rows.append(dict(part=part, fwd=fwd, mate=mate, q1=list(q1), q2=list(q2), prm=tuple(prm),
                              setting=(MODES.index(mode), cap, int(trim), insert, deltaq, offset), moves=moves_of(a1, a2),
                              score=score, contig=contig, cq=cq, stats=(ov, gaps, mism), raised=raised, built=int(cause == 0),
                              cause=cause, fixup=cls, hot=hot))
        return self.rows[-1]


def mate_of(pair):
    return P.revcomp(pair.rev)


def alignment_part(cases, rng):
    n = 0
    for prm in SCORING:
        m = maxabs(prm)
        top = 384 if m == 0 else min(384, (29999 // m - 2) // 2)
        shapes = [(top, top)] if top >= 1 else []
        shapes += [(b, b) for b in BOUND]
        shapes += [(BOUND[k], BOUND[(k + 3) % 8]) for k in range(8)] + [(BOUND[(k + 5) % 8], BOUND[k]) for k in range(8)]
        for l1, l2 in shapes:
            if not predicate(l1, l2, prm):
                continue
            p = P.make_pair(rng, l1, l2, KINDS[n % 5])
            cases.add(0, p.fwd, mate_of(p), fixed_quals(l1, n), fixed_quals(l2, 3 * n + 1), prm)
            n += 1


def predicate_part(cases, rng):
    for k, prm in enumerate(PREDICATE_ROWS):
        m = maxabs(prm)
        below, above = 29999 // m - 2, -(-30000 // m) - 2          # l1 + l2 just inside and just outside
        assert 29900 <= (below + 2) * m <= 29999 and 30000 <= (above + 2) * m <= 30100 and above <= 768
        for total in (below, above):
            l1 = min(384, total // 2 + (k % 2) * 7)
            l2 = total - l1
            p = P.make_pair(rng, l1, l2, "overlap")
            row = cases.add(1, p.fwd, mate_of(p), fixed_quals(l1, k), fixed_quals(l2, k + 5), prm)
            assert row["built"] == (1 if total == below else 0)


def fixup_part(cases, rng):
    """Search: short pairs over two letters (or four), every scoring set the predicate lets through plus the default; a pair is
    kept while a class it belongs to still has fewer than ten members."""
    have = {bit: 0 for bit in (1, 2, 4, 8, 16, 32)}
    sets = [DEFAULT, (2, -3, -1)] + SCORING
    for trial in range(40000):
        if min(have.values()) >= 10:
            break
        prm = sets[trial % len(sets)]
        l1, l2 = int(rng.integers(2, 25)), int(rng.integers(2, 25))
        if not predicate(l1, l2, prm):
            continue
        p = P.make_pair(rng, l1, l2, ("ties", "ties", "unrelated", "overlap")[trial % 4])
        fwd, mate = p.fwd, mate_of(p)
        cls = restate(fwd, mate, *prm)[3]
        if any(cls & bit and have[bit] < 10 for bit in have):
            cases.add(2, fwd, mate, fixed_quals(l1, trial), fixed_quals(l2, trial + 11), prm)
            for bit in have:
                have[bit] += bool(cls & bit)
    assert min(have.values()) >= 8, have


def contig_part(cases, rng):
    lens = (1, 2, 63, 64, 65, 128, 129, 192, 193, 256, 257, 320, 321, 383, 384)
    draw = lambda: int(lens[int(rng.integers(0, len(lens)))]) if rng.random() < 0.3 else 1 + int(384 * rng.random() ** 1.6)
    for k in range(N_CONTIGS):
        prm = SCORING[(k // 3) % len(SCORING)] if k % 3 == 2 else DEFAULT
        which = int(rng.integers(0, 3))
        offset, qmax = (33, 64, 0)[which], (93, 62, 119)[which]
        mode, cap, trim = MODES[int(rng.integers(0, 3))], (0, 40, 93)[int(rng.integers(0, 3))], bool(rng.integers(0, 2))
        insert, deltaq = ((1, 1), (20, 6), (60, 50))[int(rng.integers(0, 3))]
        l1, l2 = draw(), draw()
        if not predicate(l1, l2, prm) and rng.random() < 0.6:          # most of them shrunk until the device takes them
            room = 29999 // maxabs(prm) - 2
            l1 = max(1, min(l1, room // 2))
            l2 = max(1, min(l2, room - l1))
        kind = KINDS[int(rng.choice([0, 0, 0, 0, 1, 2, 3, 3, 4]))]
        p = P.make_pair(rng, l1, l2, kind)
        cases.add(3, with_iupac(rng, p.fwd), with_iupac(rng, mate_of(p)), run_quals(rng, l1, qmax), run_quals(rng, l2, qmax), prm,
                  mode, cap, trim, insert, deltaq, offset)


def hot_part(cases, rng):
    """Contig qualities past the byte (see the module's docstring): identical and overlapping reads with high qualities, no cap."""
    for k in range(8):
        offset, lo, hi, mode = ((0, 124, 128, "posterior"), (64, 92, 101, "sum"), (33, 108, 116, "sum"), (0, 126, 128, "posterior"))[k % 4]
        l1, l2 = int(rng.integers(20, 120)), int(rng.integers(20, 120))
        p = P.make_pair(rng, l1, l2, ("identical", "overlap")[k % 2])
        row = cases.add(4, p.fwd, mate_of(p), [int(v) for v in rng.integers(lo, hi, l1)], [int(v) for v in rng.integers(lo, hi, l2)],
                        DEFAULT, mode, 0, False, 20, 6, offset)
        assert row["cause"] == 2, (k, max(row["cq"]))
    for kind in ("identical", "overlap"):                # ... and exactly on it: 127 + 128 at offset 0 is the byte 255, which the
        p = P.make_pair(rng, 60, 50, kind)               # device builds and the text filter then refuses (Q255 has no code)
        row = cases.add(4, p.fwd, mate_of(p), [127] * 60, [128] * 50, DEFAULT, "sum", 0, False, 20, 6, 0)
        assert row["built"] and max(row["cq"]) == 255


def cat_text(strs):
    off = np.zeros(len(strs) + 1, np.int64)
    off[1:] = np.cumsum([len(s) for s in strs])
    return np.frombuffer("".join(strs).encode("ascii"), np.uint8).copy(), off


def cat_ints(lists, dtype):
    off = np.zeros(len(lists) + 1, np.int64)
    off[1:] = np.cumsum([len(v) for v in lists])
    flat = np.concatenate([np.asarray(v, np.int64) for v in lists]) if lists else np.zeros(0, np.int64)
    assert flat.size == 0 or (np.iinfo(dtype).min <= flat.min() and flat.max() <= np.iinfo(dtype).max)
    return flat.astype(dtype), off


def write_archive(path, arrays):
    """np.savez_compressed with a fixed timestamp on every member: the same arrays give the same bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for name, arr in arrays.items():
            raw = io.BytesIO()
            np.lib.format.write_array(raw, np.ascontiguousarray(arr), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, raw.getvalue(), compresslevel=9)


def main():
    pyref, tmp = MG.load_python_reference()
    try:
        nw = MG.load_cython_nw(tmp)
        cases = Cases(nw, pyref)
        alignment_part(cases, np.random.default_rng(20241101))
        predicate_part(cases, np.random.default_rng(20241102))
        fixup_part(cases, np.random.default_rng(20241103))
        contig_part(cases, np.random.default_rng(20241104))
        hot_part(cases, np.random.default_rng(20241105))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    rows = cases.rows
    # ---- the conditions (not measurements) ----
    contigs = [r for r in rows if r["part"] in (3, 4)]
    built = [r for r in rows if r["built"]]
    share = sum(r["built"] for r in contigs) / len(contigs)
    assert share >= 0.80, share
    causes = {c: sum(1 for r in contigs if r["cause"] == c) for c in (1, 2, 3, 4)}
    assert min(causes[1], causes[2], causes[3]) >= 5, causes
    assert {(len(r["mate"]) + 63) // 64 for r in built if r["part"] == 3} == {1, 2, 3, 4, 5, 6}
    assert any(q > 93 for r in built for q in r["cq"])
    assert sum(r["hot"] for r in built) >= 100
    assert all(sum(1 for r in rows if r["fixup"] & bit) >= 8 for bit in (1, 2, 4, 8, 16, 32))
    assert {r["prm"] for r in rows if r["part"] == 0} == set(SCORING)
    assert set("".join(r["fwd"] + r["mate"] for r in contigs)) == set("ACGT" + IUPAC)
    # ---- the arrays ----
    fwd, foff = cat_text([r["fwd"] for r in rows])
    mate, moff = cat_text([r["mate"] for r in rows])
    contig, coff = cat_text([r["contig"] for r in rows])
    q1, _ = cat_ints([r["q1"] for r in rows], np.uint8)
    q2, _ = cat_ints([r["q2"] for r in rows], np.uint8)
    cq, _ = cat_ints([r["cq"] for r in rows], np.int16)
    moves, aoff = cat_ints([r["moves"] for r in rows], np.uint8)
    arrays = dict(fwd=fwd, foff=foff, mate=mate, moff=moff, q1=q1, q2=q2, moves=moves, aoff=aoff, contig=contig, coff=coff, cq=cq,
                  score=np.array([r["score"] for r in rows], np.int64), prm=np.array([r["prm"] for r in rows], np.int32),
                  setting=np.array([r["setting"] for r in rows], np.int32), stats=np.array([r["stats"] for r in rows], np.int32),
                  part=np.array([r["part"] for r in rows], np.int8), raised=np.array([r["raised"] for r in rows], np.int8),
                  built=np.array([r["built"] for r in rows], np.int8), cause=np.array([r["cause"] for r in rows], np.int8),
                  fixup=np.array([r["fixup"] for r in rows], np.int8))
    out = os.path.join(HERE, "nw_domain.npz")
    write_archive(out, arrays)
    size = os.path.getsize(out)
    assert size <= SIZE_LIMIT, size
    per_part = {p: sum(1 for r in rows if r["part"] == p) for p in range(5)}
    print("nw_domain      n=%d cases %s, %.1f %% of the contig cases built, hand-back causes %s, posterior look-ups above 41: %d, "
          "reference raised: %d, %d bytes -> %s"
          % (len(rows), per_part, 100 * share, causes, sum(r["hot"] for r in built), sum(r["raised"] for r in rows), size,
             os.path.relpath(out, ROOT)))


if __name__ == "__main__":
    main()
