"""Writes tests/golden/contig_random_pairs.json: the reference's own reverse_complement and make_contig (moira/moira.py, loaded
through make_golden.load_python_reference) on the seeded random pairs of tests/test_contig.py, each contig built on the alignment
moira_amd.contig.nw_align gives.  Run where the reference checkout exists:

    python tests/golden/make_contig_pairs.py
"""
import json
import os
import shutil
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), HERE]

import make_golden as MG                                    # noqa: E402
from moira_amd import contig as CT                          # noqa: E402
from test_contig import CONTIG_MODES, _random_pair          # noqa: E402


def main():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        M, tmp = MG.load_python_reference()
    try:
        rng = np.random.default_rng(11)
        pairs = []
        for _ in range(60):
            f, fq, r, rq = _random_pair(rng)
            rrc, rrq = M.reverse_complement(r, list(rq))
            a1, a2, _ = CT.nw_align(f, rrc, 1, -1, -2)
            contigs = [list(M.make_contig(a1, list(fq), a2, list(rrq), 20, 6, mode, cap, trim)) for mode, cap, trim in CONTIG_MODES]
            pairs.append({"f": f, "fq": fq, "r": r, "rq": rq, "rc": [rrc, list(rrq)], "contigs": contigs})
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    out = os.path.join(HERE, "contig_random_pairs.json")
    with open(out, "w") as fh:
        json.dump({"source": "moira/moira.py reverse_complement and make_contig (lib2to3 copy), insert 20, deltaq 6",
                   "modes": [list(m) for m in CONTIG_MODES], "pairs": pairs}, fh, separators=(",", ":"))
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
