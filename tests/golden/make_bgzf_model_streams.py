"""Writes tests/golden/bgzf_model_streams.json: what the host lane model of k_bgzf_deflate (tests/helpers/bgzf_lane_check.cpp, built
here with g++ -O2 and no sanitizer) gives for every member of every input of tests/helpers/bgzf_model.all_inputs() -- n, btype,
the stream's length and SHA-256, literals, matches, matched.  Every input is seeded: a second run leaves the file unchanged.
tests/test_bgzf_model_streams.py recomputes it, tests/test_gpu_bgzf.py holds the device's bytes to it.

    python tests/golden/make_bgzf_model_streams.py
"""
import os
import shutil
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "tests")]

from helpers import bgzf_model as M                         # noqa: E402


def main():
    tmp = tempfile.mkdtemp(prefix="bgzf_model_")
    try:
        exe = M.build(os.path.join(tmp, "check"))
        entries, _ = M.compute(exe, tmp, M.all_inputs())
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    text = M.dumps(entries)
    old = open(M.FIXTURE).read() if os.path.exists(M.FIXTURE) else None
    if old != text:
        with open(M.FIXTURE, "w") as fh:
            fh.write(text)
    members = sum(len(v) for v in entries.values())
    print("%s: %d inputs, %d members, %d bytes, %s" % (os.path.relpath(M.FIXTURE, ROOT), len(entries), members, len(text),
                                                       "unchanged" if old == text else "written"))


if __name__ == "__main__":
    main()
