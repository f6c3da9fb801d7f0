"""Read pairs for the device contig tests (tests/test_contig_device_model.py, tests/test_gpu_contigs.py): the reference
fixtures (nw_pairs / nw_contigs, and nw_domain: the edges of the domain) as FASTQ-like texts with record indexes, generated pairs
of chosen lengths and kinds, and the host's answers (moira_amd.contig: mct_nw_align / mct_contigs_from_fastq)."""
import numpy as np

import golden_io as G

COMP = {"A": "T", "C": "G", "T": "A", "G": "C", "N": "N", "W": "W", "S": "S", "R": "Y", "Y": "R", "M": "K", "K": "M", "B": "V",
        "V": "B", "D": "H", "H": "D", "-": "-", ".": "."}
MODES = {"best": 0, "sum": 1, "posterior": 2}


def revcomp(s):
    return "".join(COMP[c] for c in reversed(s))


class Pair:
    """One read pair as the FASTQ files hold it: fwd / rev are the records' sequence lines (rev NOT yet reverse-complemented),
    fq / rq their quality lines as bytes (q + offset)."""

    def __init__(self, fwd, fq, rev, rq, name="p"):
        self.fwd, self.fq, self.rev, self.rq, self.name = fwd, bytes(fq), rev, bytes(rq), name


def texts(pairs):
    """-> (fbuf uint8, fidx int64[n, 6], rbuf, ridx): records at unaligned offsets, the last quality line ends the text."""
    def one(records):
        parts, idx, pos = [], np.zeros((len(records), 6), np.int64), 0
        for i, (name, seq, qual) in enumerate(records):
            head = b"@" + name.encode() + b" extra\n"
            idx[i] = (pos + 1, len(name), pos + len(head), len(seq), pos + len(head) + len(seq) + 3, len(qual))
            rec = head + seq + b"\n+\n" + qual + (b"\n" if i + 1 < len(records) else b"")
            parts.append(rec)
            pos += len(rec)
        return np.frombuffer(b"".join(parts), np.uint8).copy(), idx
    fbuf, fidx = one([("%s%d" % (p.name, i), p.fwd.encode("latin-1"), p.fq) for i, p in enumerate(pairs)])
    rbuf, ridx = one([("%s%d" % (p.name, i), p.rev.encode("latin-1"), p.rq) for i, p in enumerate(pairs)])
    return fbuf, fidx, rbuf, ridx


def _strings(buf, off):
    b = buf.tobytes().decode("ascii")
    return [b[off[i]:off[i + 1]] for i in range(len(off) - 1)]


_cache = {}


def fixture_alignments():
    """tests/golden/nw_pairs.npz -> [(Pair, (match, mismatch, gap), aln1, aln2, score)], 4,808 of them; the reverse record is the
    reverse complement of the fixture's second sequence, qualities 2..41 from a fixed stream at offset 33."""
    if "aln" not in _cache:
        z = G.load_set("nw_pairs")
        s1, s2 = _strings(z["seq1"], z["off1"]), _strings(z["seq2"], z["off2"])
        a1, a2 = _strings(z["aln1"], z["aoff1"]), _strings(z["aln2"], z["aoff2"])
        rng = np.random.default_rng(20240607)
        out = []
        for k in range(len(s1)):
            fq = (rng.integers(2, 42, len(s1[k])) + 33).astype(np.uint8).tobytes()
            rq = (rng.integers(2, 42, len(s2[k])) + 33).astype(np.uint8).tobytes()
            out.append((Pair(s1[k], fq, revcomp(s2[k]), rq), tuple(int(v) for v in z["params"][z["param"][k]]), a1[k], a2[k],
                        int(z["score"][k])))
        _cache["aln"] = out
    return _cache["aln"]


def fixture_contigs():
    """tests/golden/nw_contigs.npz -> (rows, insert, deltaq); rows = [(Pair, (match, mismatch, gap), consensus name, cap, trim,
    contig, contig quality bytes at offset 33, (overlap, gaps, mismatches))], 2,565 of them.  The reverse record carries the
    fixture's q2 reversed (the fixture's q2 runs along the reverse-complemented mate)."""
    if "contigs" not in _cache:
        z, c = G.load_set("nw_pairs"), G.load_set("nw_contigs")
        s1, s2 = _strings(z["seq1"], z["off1"]), _strings(z["seq2"], z["off2"])
        contigs = _strings(c["contig"], c["coff"])
        rows = []
        for r in range(len(contigs)):
            k, mi = int(c["pair"][r]), int(c["mode"][r])
            q1 = c["q1"][c["q1off"][r]:c["q1off"][r + 1]].astype(np.int64)
            q2 = c["q2"][c["q2off"][r]:c["q2off"][r + 1]].astype(np.int64)
            cq = c["cq"][c["cqoff"][r]:c["cqoff"][r + 1]].astype(np.int64)
            rows.append((Pair(s1[k], (q1 + 33).astype(np.uint8).tobytes(), revcomp(s2[k]), (q2[::-1] + 33).astype(np.uint8).tobytes()),
                         tuple(int(v) for v in z["params"][z["param"][k]]), str(c["modes"][mi]), int(c["caps"][mi]), bool(c["trims"][mi]),
                         contigs[r], (cq + 33).astype(np.uint8).tobytes(), tuple(int(v) for v in c["stats"][r])))
        _cache["contigs"] = (rows, int(c["insert"]), int(c["deltaq"]))
    return _cache["contigs"]


def fixture_settings():
    """The five (consensus, cap, trim) settings of nw_contigs.npz."""
    c = G.load_set("nw_contigs")
    return [(str(m), int(cap), bool(t)) for m, cap, t in zip(c["modes"], c["caps"], c["trims"])]


class DomainCase:
    """One case of tests/golden/nw_domain.npz: the pair as the FASTQ files hold it (qualities at the case's offset), every
    parameter, and the REFERENCE's answers -- aln1 / aln2 / score (the Cython aligner), contig / cq (quality bytes at the offset;
    None where a quality leaves its byte) / stats (make_contig).  built: the device must build it; cause: 0, or why it must hand
    the pair back (1 the 16-bit predicate, 2 a contig quality above its byte, 3 below zero, 4 the reference raised); part and
    fixup: see tests/golden/make_nw_domain.py."""

    def group(self):
        """What one device call fixes: (scoring, consensus, cap, trim, insert, deltaq, offset)."""
        return (self.prm, self.mode, self.cap, self.trim, self.insert, self.deltaq, self.offset)


def fixture_domain():
    """tests/golden/nw_domain.npz -> [DomainCase]: the edges of the domain (scoring up to the 16-bit predicate, zero / negative /
    positive parameters, every IUPAC letter, offsets 0 / 33 / 64, qualities up to 128, every consensus setting), from the reference."""
    if "domain" not in _cache:
        z = G.load_set("nw_domain")
        fwd, mate, contig = _strings(z["fwd"], z["foff"]), _strings(z["mate"], z["moff"]), _strings(z["contig"], z["coff"])
        out = []
        for k in range(len(fwd)):
            c = DomainCase()
            c.k, c.part, c.fixup, c.built, c.cause, c.raised = k, int(z["part"][k]), int(z["fixup"][k]), bool(z["built"][k]), int(z["cause"][k]), bool(z["raised"][k])
            c.prm = tuple(int(v) for v in z["prm"][k])
            mode, c.cap, trim, c.insert, c.deltaq, c.offset = (int(v) for v in z["setting"][k])
            c.mode, c.trim = ("best", "sum", "posterior")[mode], bool(trim)
            c.q1 = z["q1"][z["foff"][k]:z["foff"][k + 1]].astype(np.int64)
            c.q2 = z["q2"][z["moff"][k]:z["moff"][k + 1]].astype(np.int64)               # along the mate as it aligns
            c.mate = mate[k]
            c.pair = Pair(fwd[k], (c.q1 + c.offset).astype(np.uint8).tobytes(), revcomp(mate[k]), (c.q2[::-1] + c.offset).astype(np.uint8).tobytes())
            a1, a2, u, v = [], [], 0, 0
            for mv in z["moves"][z["aoff"][k]:z["aoff"][k + 1]]:                         # 0 both reads, 1 the forward read alone, 2 the mate alone
                a1.append(fwd[k][u] if mv != 2 else "-"); u += mv != 2
                a2.append(mate[k][v] if mv != 1 else "-"); v += mv != 1
            assert (u, v) == (len(fwd[k]), len(mate[k]))
            c.aln1, c.aln2, c.score = "".join(a1), "".join(a2), int(z["score"][k])
            c.contig, c.stats = contig[k], tuple(int(v) for v in z["stats"][k])
            c.cq_ints = z["cq"][z["coff"][k]:z["coff"][k + 1]].astype(np.int64)
            fits = len(c.cq_ints) == 0 or (c.cq_ints.min() >= 0 and c.cq_ints.max() + c.offset <= 255)
            c.cq = (c.cq_ints + c.offset).astype(np.uint8).tobytes() if fits else None
            out.append(c)
        _cache["domain"] = out
    return _cache["domain"]


def make_pair(rng, l1, l2, kind, qlo=2, qhi=42):
    """A pair of the given lengths: 'overlap' (the mate's reverse complement continues the forward read, 3 % errors), 'ties'
    (two letters, tie-heavy), 'unrelated', 'contained' (the shorter read lies inside the longer), 'identical'."""
    alpha = "AC" if kind == "ties" else "ACGT"
    rnd = lambda n: "".join(alpha[int(v)] for v in rng.integers(0, len(alpha), n))
    fwd = rnd(l1)
    if kind in ("unrelated", "ties"):
        mate = rnd(l2)                                  # the mate as it aligns (already reverse-complemented)
    elif kind == "identical":
        mate = (fwd * (l2 // l1 + 1))[:l2]
    elif kind == "contained":
        if l2 <= l1:
            st = int(rng.integers(0, l1 - l2 + 1))
            mate = fwd[st:st + l2]
        else:
            st = int(rng.integers(0, l2 - l1 + 1))
            mate = rnd(st) + fwd + rnd(l2 - l1 - st)
    else:                                               # overlap: the mate starts inside the forward read and runs past its end
        ov = max(1, min(l1, l2) * 2 // 3)
        mate = (fwd[l1 - ov:] + rnd(l2))[:l2]
    if kind in ("overlap", "contained"):
        m = list(mate)
        for pos in np.nonzero(rng.random(l2) < 0.03)[0]:
            m[pos] = "ACGT"[("ACGT".index(m[pos]) + 1 + int(rng.integers(0, 3))) % 4]
        mate = "".join(m)
    fq = (rng.integers(qlo, qhi, l1) + 33).astype(np.uint8).tobytes()
    rq = (rng.integers(qlo, qhi, l2) + 33).astype(np.uint8).tobytes()
    return Pair(fwd, fq, revcomp(mate), rq)


def host_alignment(pair, match, mismatch, gap):
    from moira_amd import contig as CT
    return CT.nw_align(pair.fwd, revcomp(pair.rev), match, mismatch, gap)


def host_contigs(pairs, offset=33, match=1, mismatch=-1, gap=-2, insert=20, deltaq=6, consensus="best", cap=40, trim=False):
    """mct_contigs_from_fastq on the pairs -> (fbuf, fidx, rbuf, ridx, cbuf, cidx, aux)."""
    from moira_amd import contig as CT
    fbuf, fidx, rbuf, ridx = texts(pairs)
    cbuf, cidx, aux = CT.contigs_from_fastq(fbuf, fidx, rbuf, ridx, offset, match, mismatch, gap, insert, deltaq, consensus, cap, trim,
                                            threads=4)
    return fbuf, fidx, rbuf, ridx, cbuf, cidx, aux


def records(cbuf, cidx):
    """[(header, contig, quality bytes)] of a contig buffer + index: the defined bytes of every slot."""
    b = cbuf.tobytes() if isinstance(cbuf, np.ndarray) else bytes(cbuf)
    return [(b[r[0]:r[0] + r[1]], b[r[2]:r[2] + r[3]], b[r[4]:r[4] + r[5]]) for r in np.asarray(cidx)]
