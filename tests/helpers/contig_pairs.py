"""Read pairs for the device contig tests (tests/test_contig_device_model.py, tests/test_gpu_contigs.py): the two reference
fixtures as FASTQ-like texts with record indexes, generated pairs of chosen lengths and kinds, and the host's answers
(moira_amd.contig: mct_nw_align / mct_contigs_from_fastq)."""
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
