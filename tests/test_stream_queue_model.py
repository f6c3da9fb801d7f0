"""StreamQueue (moira_amd/csrc/mpb_queue.h), the queue discipline of the staged host entries, without a device:
tests/helpers/stream_queue_check.cpp is the header's second includer, with a runtime that records every call and fails the ones it
is told to.  Built with -fsanitize=address,undefined and run as a program; nothing is preloaded.  The program drives one script (up,
up, zero, a run with two launches, down, down, wait, up, wait) with no failure, with every single failing call and with pairs of
them, and the scopes that matter to the destructor; the sensitivity build's destructor does nothing and must fail."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(tmp, *defines):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = os.path.join(str(tmp), "check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "moira_amd", "csrc")] + list(defines) +
                          [os.path.join(ROOT, "tests", "helpers", "stream_queue_check.cpp"), "-o", exe])
    return exe


def run(exe):
    r = subprocess.run([exe], capture_output=True, text=True)
    out = r.stdout + r.stderr[-3000:]
    counts = {m.group(1): (int(m.group(2)), int(m.group(3))) for m in re.finditer(r"^(\w+): (\d+) checks, (\d+) failed$", out, re.M)}
    return r.returncode, out, counts


@pytest.fixture(scope="module")
def result(tmp_path_factory):
    return run(build(tmp_path_factory.mktemp("stream_queue")))


def test_the_script_holds_for_no_failure_every_failing_call_and_pairs_of_them(result):
    rc, out, counts = result
    assert rc == 0 and "FAIL" not in out, out
    # 1 + 9 calls x 3 errors + 2 x 21 pairs runs of the script, five checks each
    assert counts["script"] == (5 * (1 + 27 + 42), 0), out


def test_the_destructor_waits_for_what_is_pending_and_for_nothing_else(result):
    rc, out, counts = result
    assert rc == 0 and counts["destructor"] == (9, 0), out


def test_a_destructor_that_does_nothing_fails_the_destructor_checks_alone(tmp_path):
    rc, out, counts = run(build(tmp_path, "-DSTREAM_QUEUE_NO_DTOR_SYNC"))
    assert rc == 1, out
    # the five scopes left with something queued since the last wait; the four that must not synchronise still hold
    assert counts["script"][1] == 0 and counts["destructor"] == (9, 5), out
    assert len(re.findall(r"^FAIL destructor: .* when the scope is left", out, re.M)) == 5, out
