"""the shipped kernel file carries no experiment switches; every experiment build is a set of exact text patches of a
COPY of it (tools/experiments/make_variant.py).  Here: the shipped file has no conditional compilation at all, and every variant's
patches still apply (each exactly once) and the patched copy still parses and instantiates for gfx950 (device-side syntax-only
pass: about 1.5 s per variant; the GPU box builds and runs them)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAKE = os.path.join(ROOT, "tools", "experiments", "make_variant.py")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def variants():
    r = subprocess.run([sys.executable, MAKE, "--list"], capture_output=True, text=True, check=True)
    return r.stdout.split()


def test_the_shipped_kernels_have_no_conditional_compilation():
    src = open(os.path.join(ROOT, "moira_amd", "csrc", "mpb_kernels.hip")).read().splitlines()
    assert [l for l in src if l.startswith(("#if", "#ifdef", "#ifndef", "#elif"))] == []
    from moira_amd.build import HOST_SOURCES
    assert len(HOST_SOURCES) >= 7 and all(os.path.dirname(p) == os.path.join(ROOT, "moira_amd", "csrc") for p in HOST_SOURCES)
    for path in HOST_SOURCES:            # every host unit of the library, the broker among them
        assert "MPB_TUNING_KNOBS" not in open(path).read(), path
    assert len(variants()) >= 4


@pytest.mark.parametrize("name", variants())
def test_variant_applies_and_parses_for_gfx950(name, tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc here")
    out = str(tmp_path / (name + ".hip"))
    r = subprocess.run([sys.executable, MAKE, name, out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert open(out).read() != open(os.path.join(ROOT, "moira_amd", "csrc", "mpb_kernels.hip")).read()
    c = subprocess.run([HIPCC, "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                        "--cuda-device-only", "-fsyntax-only", out], capture_output=True, text=True, timeout=300)
    assert c.returncode == 0, c.stderr[-3000:]
