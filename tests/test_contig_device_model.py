"""The device contig builder's per-lane code on the host (moira_amd/csrc/mpb_contig_lane.inc through
tests/helpers/contig_device_check.cpp): 64 lane states in lockstep with checked loads must reproduce the REFERENCE's
alignments (tests/golden/nw_pairs.npz) and contigs (nw_contigs.npz), hand nothing of them back, and hand a pair with a
damaged descriptor back without one load outside the buffers; on the edges of the domain (nw_domain.npz) they must give the
reference's answers for every case the device has to build and hand every other case back.  The kernel itself:
tests/test_gpu_contigs.py."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from helpers import contig_pairs as P
from moira_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_CORRUPT = 11


def build_checker(exe, *flags):
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "moira_amd", "csrc"),
                           os.path.join(ROOT, "tests", "helpers", "contig_device_check.cpp"), "-o", exe] + (list(flags) or ["-O2"]))
    return exe


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    return build_checker(str(tmp_path_factory.mktemp("contig_model") / "check"))


def tables():
    t = np.empty((2, 256, 256), np.int32)
    assert L.load().mpb_contig_posterior_tables(t[0].ctypes.data, t[1].ctypes.data) == 0
    return t


def write_cases(path, cases):
    blob = [tables().tobytes(), struct.pack("<i", len(cases))]
    for p, (m, mm, g), insert, deltaq, mode, cap, trim, offset, corrupt in cases:
        blob.append(struct.pack("<12i", len(p.fwd), len(p.rev), m, mm, g, insert, deltaq, P.MODES[mode], cap, int(trim), offset, corrupt))
        blob += [p.fwd.encode("latin-1"), p.fq, p.rev.encode("latin-1"), p.rq]
    with open(path, "wb") as f:
        f.write(b"".join(blob))


def run_checker(exe, fin, fout, n):
    """-> ([dict per case], the checker's summary line, the output file's bytes)."""
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    raw, pos, out = open(fout, "rb").read(), 0, []
    for _ in range(n):
        done, alen, score, clen, ov, gaps, mism = struct.unpack_from("<7i", raw, pos)
        pos += 28
        a1, a2 = raw[pos:pos + alen], raw[pos + alen:pos + 2 * alen]
        pos += 2 * alen
        contig, cq = raw[pos:pos + clen], raw[pos + clen:pos + 2 * clen]
        pos += 2 * clen
        out.append(dict(done=done, aln1=a1.decode("latin-1"), aln2=a2.decode("latin-1"), score=score, contig=contig.decode("latin-1"),
                        cq=cq, stats=(ov, gaps, mism)))
    assert pos == len(raw)
    return out, r.stdout.strip(), raw


def run_model(exe, tmp, cases):
    """cases: [(Pair, (match, mismatch, gap), insert, deltaq, consensus name, cap, trim, offset, corrupt)] ->
    ([dict per case], the checker's summary line)."""
    fin, fout = os.path.join(tmp, "cases.bin"), os.path.join(tmp, "out.bin")
    write_cases(fin, cases)
    return run_checker(exe, fin, fout, len(cases))[:2]


def test_lane_code_reproduces_the_reference_alignments(checker, tmp_path):
    """All 4,808 alignments and scores of nw_pairs.npz (the reference's Cython aligner): tie-break order, the 3' fix-up, the score
    as the sum of the path's cells.  Every fixture pair is eligible (lengths 1..328, predicate at most 5,920): done is all ones."""
    fx = P.fixture_alignments()
    assert len(fx) == 4808
    lens = [len(p.fwd) for p, *_ in fx] + [len(p.rev) for p, *_ in fx]
    assert min(lens) >= 1 and max(lens) <= 328
    assert max((len(p.fwd) + len(p.rev) + 2) * max(abs(v) for v in prm) for p, prm, *_ in fx) < 30000
    got, line = run_model(checker, str(tmp_path), [(p, prm, 20, 6, "best", 40, False, 33, 0) for p, prm, *_ in fx])
    assert "0 handed back, 0 loads out of bounds, 0 differ" in line, line
    bad = [k for k, (g, (_, _, a1, a2, sc)) in enumerate(zip(got, fx)) if (g["done"], g["aln1"], g["aln2"], g["score"]) != (1, a1, a2, sc)]
    assert not bad, bad[:10]


def test_lane_code_reproduces_the_reference_contigs(checker, tmp_path):
    """All 2,565 contigs of nw_contigs.npz (moira.py's make_contig on the reference's own alignments; best / sum / posterior, caps,
    trim): the reverse record is fed as the reverse complement of seq2 with reversed qualities, at offset 33.  Qualities are
    2..41 and contig qualities at most 82, so nothing is handed back."""
    rows, insert, deltaq = P.fixture_contigs()
    assert len(rows) == 2565
    got, line = run_model(checker, str(tmp_path), [(p, prm, insert, deltaq, mode, cap, trim, 33, 0) for p, prm, mode, cap, trim, *_ in rows])
    assert "0 handed back, 0 loads out of bounds, 0 differ" in line, line
    bad = [k for k, (g, row) in enumerate(zip(got, rows)) if (g["done"], g["contig"], g["cq"], g["stats"]) != (1, row[5], row[6], row[7])]
    assert not bad, bad[:10]


def test_a_damaged_descriptor_is_handed_back_without_a_load_out_of_bounds(checker, tmp_path):
    """Host only (never provoked on a GPU): every way of damaging a descriptor -- offsets past or before a text, lengths outside
    1..384, a header that does not fit rec_cap -- gives done = 0 and no checked load fails; the intact descriptor is built."""
    rng = np.random.default_rng(5)
    pairs = [P.make_pair(rng, l1, l2, "overlap") for l1, l2 in ((1, 1), (37, 90), (250, 251), (384, 384))]
    cases = [(p, (1, -1, -2), 20, 6, "best", 40, False, 33, c) for p in pairs for c in range(N_CORRUPT + 1)]
    got, line = run_model(checker, str(tmp_path), cases)
    assert "0 loads out of bounds, 0 differ" in line, line
    for (p, _, _, _, _, _, _, _, c), g in zip(cases, got):
        assert g["done"] == (1 if c == 0 else 0), (len(p.fwd), len(p.rev), c)


def test_lane_code_equals_the_host_on_the_size_class_edges(checker, tmp_path):
    """Lengths at the C boundaries (64 columns per lane step) and at 384, every sequence kind: alignment, score and contig as
    the host library builds them."""
    from moira_amd import contig as CT
    rng = np.random.default_rng(11)
    edge = (1, 2, 63, 64, 65, 128, 129, 192, 193, 256, 257, 320, 321, 383, 384)
    kinds = ("overlap", "ties", "unrelated", "contained", "identical")
    cases = []
    for n, l1 in enumerate(edge):
        for m, l2 in enumerate(edge):
            if (n + m) % 3 == 0:
                prm = ((1, -1, -2), (2, -3, -1), (1, 0, 0))[(n + 2 * m) % 3]
                mode = ("best", "sum", "posterior")[(n + m) % 3]
                cases.append((P.make_pair(rng, l1, l2, kinds[(n * 7 + m) % 5]), prm, 20, 6, mode, 40 if n % 2 else 0, bool(m % 2), 33, 0))
    got, line = run_model(checker, str(tmp_path), cases)
    assert "0 handed back, 0 loads out of bounds, 0 differ" in line, line
    for (p, prm, insert, deltaq, mode, cap, trim, _, _), g in zip(cases, got):
        a1, a2, sc = P.host_alignment(p, *prm)
        assert (g["aln1"], g["aln2"], g["score"]) == (a1, a2, sc), (len(p.fwd), len(p.rev), prm)
        fq = [b - 33 for b in p.fq]
        rq = [b - 33 for b in p.rq][::-1]
        contig, cq, ov, gaps, mism = CT.make_contig(a1, fq, a2, rq, insert, deltaq, mode, cap, trim)
        assert (g["contig"], list(g["cq"]), g["stats"]) == (contig, [q + 33 for q in cq], (ov, gaps, mism)), (len(p.fwd), len(p.rev), mode)


# ---- the edges of the domain: tests/golden/nw_domain.npz ----------------------------------------------------------------------

def domain_cases():
    return [(c.pair, c.prm, c.insert, c.deltaq, c.mode, c.cap, c.trim, c.offset, 0) for c in P.fixture_domain()]


def domain_mismatches(got):
    """The fixture's cases the model's answers `got` disagree with: a built case must give the REFERENCE's strings, score, contig,
    quality bytes and statistics, every other case done == 0."""
    bad = []
    for c, g in zip(P.fixture_domain(), got):
        want = (1, c.aln1, c.aln2, c.score, c.contig, c.cq, c.stats) if c.built else (0,)
        have = (g["done"], g["aln1"], g["aln2"], g["score"], g["contig"], g["cq"], g["stats"]) if c.built else (g["done"],)
        if have != want:
            bad.append(c.k)
    return bad


@pytest.fixture(scope="module")
def domain_run(checker, tmp_path_factory):
    """The model over the whole fixture, once: (cases file, [dict per case], summary line, output bytes)."""
    tmp = tmp_path_factory.mktemp("contig_domain")
    fin = str(tmp / "cases.bin")
    write_cases(fin, domain_cases())
    return (fin,) + run_checker(checker, fin, str(tmp / "out.bin"), len(P.fixture_domain()))


def test_lane_code_reproduces_the_reference_on_the_edges_of_the_domain(domain_run):
    """tests/golden/nw_domain.npz (tests/golden/make_nw_domain.py): scoring up to the 16-bit predicate and on both sides of it,
    zero / negative / sign-reversed parameters, every outcome of the 3' fix-up, fifteen IUPAC letters, offsets 0 / 33 / 64,
    qualities 0..128, every consensus / cap / trim / insert / deltaq setting.  Built cases: the reference's answers; a case whose
    contig quality leaves its byte or falls below zero, or that the predicate refuses: handed back."""
    _, got, line, _ = domain_run
    fx = P.fixture_domain()
    assert len(fx) >= 1000 and {c.cause for c in fx} >= {0, 1, 2, 3} and not any(c.raised for c in fx)
    assert "%d cases, %d handed back, 0 loads out of bounds, 0 differ between fills" % (len(fx), sum(not c.built for c in fx)) in line, line
    bad = domain_mismatches(got)
    assert not bad, bad[:10]


def test_sanitizer_build_of_the_model_on_the_edges_of_the_domain(domain_run, tmp_path):
    """The same stand-alone program built with -fsanitize=address,undefined (its LDS block is a heap block of exactly
    cd_lds_bytes, its text buffers end where the kernel's do) on the same cases file: no report, the same output bytes."""
    fin, _, _, raw = domain_run
    exe = build_checker(str(tmp_path / "check_san"), "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    _, line, raw_san = run_checker(exe, fin, str(tmp_path / "out.bin"), len(P.fixture_domain()))
    assert "0 loads out of bounds, 0 differ between fills" in line, line
    assert raw_san == raw


VARIANTS = {1: "the column wins the fix-up on cs >= rs", 2: "the first maximum of the last column / row, not the last",
            3: "posterior tables clamped to qualities of 41 or less"}


@pytest.mark.parametrize("variant", sorted(VARIANTS), ids=lambda v: "variant%d" % v)
def test_a_wrong_model_fails_the_domain_fixture(domain_run, tmp_path, variant):
    """Sensitivity, on the CPU: the checker built with -DCD_CHECK_VARIANT (a deliberately wrong fix-up rule, scan or table) must
    disagree with the fixture, and in the case classes made for it.  (nw_pairs.npz notices variants 1 and 2 as well, under its
    five plain scoring sets; here they also fail under negative, zero and near-boundary scoring.  Variant 3 passes both older
    fixtures, whose qualities end at 41.)"""
    fin = domain_run[0]
    fx = P.fixture_domain()
    exe = build_checker(str(tmp_path / "check_variant"), "-O2", "-DCD_CHECK_VARIANT=%d" % variant)
    got, _, _ = run_checker(exe, fin, str(tmp_path / "out.bin"), len(fx))
    bad = [fx[k] for k in domain_mismatches(got)]
    assert bad, VARIANTS[variant]
    if variant == 1:                                     # exactly the cases with equal maxima can change, and some do
        assert all(c.fixup & 8 for c in bad)
    elif variant == 2:                                   # a maximum held twice, under scoring the older fixtures do not have
        assert any(c.fixup & 16 for c in bad) and any(c.fixup & 32 for c in bad)
        assert any(max(abs(v) for v in c.prm) > 10 or min(c.prm) >= 0 or max(c.prm) <= 0 for c in bad)
    else:                                                # only posterior cases with a quality above 41 -- which nw_contigs.npz
        assert all(c.mode == "posterior" and max(c.q1.max(), c.q2.max()) > 41 for c in bad)       # does not hold: it passes
        rows, insert, deltaq = P.fixture_contigs()
        old, _ = run_model(exe, str(tmp_path), [(p, prm, insert, deltaq, mode, cap, trim, 33, 0) for p, prm, mode, cap, trim, *_ in rows])
        assert all((g["done"], g["contig"], g["cq"], g["stats"]) == (1, row[5], row[6], row[7]) for g, row in zip(old, rows))
