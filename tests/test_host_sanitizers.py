"""The host sanitizer scripts build and run clean: tools/tsan_poisson.sh (ThreadSanitizer on the Poisson host tail, two threads
reaching the factorial table at once) and tools/asan_api.sh (AddressSanitizer + UBSan on the packers, the threaded tail and the
argument checks).  Both compile the HIP-free unit of the C ABI layer (moira_amd/csrc/mpb_hostonly.cpp) plus a main of their own
into a stand-alone program; nothing is loaded into this process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_script(name, tmp_path):
    env = dict(os.environ, TMPDIR=str(tmp_path))
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", name)], capture_output=True, text=True, env=env, timeout=600)
    print(r.stdout)
    print(r.stderr)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return r.stdout


def test_tsan_poisson(tmp_path):
    out = run_script("tsan_poisson.sh", tmp_path)
    assert "tsan_poisson: rc 0 0, results identical: 1" in out


def test_asan_api(tmp_path):
    out = run_script("asan_api.sh", tmp_path)
    assert "asan_api: 0 failed checks" in out
