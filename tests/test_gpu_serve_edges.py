"""Directed inputs for the resident per-read kernel (k_serve): every read of tests/helpers/serve_cells.py -- each crossing row of
the register-resident body of small_one_read, each tail length of its first, second and last chunk, reads whose prediction is too
small, reads it must hand back, both sides of every gate it sits behind, the thin bodies as k_serve runs them -- through every way a
per-read call is served, bit for bit against the oracle on ee and Ns: the in-process entry (k_serve with one mailbox entry), the
launch per call (MPB_SERVE=0), the broker's three forms with one client and its direct form with three.  Which body ran shows in
the broker's `solo` count (reads that came back with pass = 2 and were run alone): it is asserted from the cells.  A forged length
word puts bytes that are not the identity step behind a read's end inside its last chunk, where only the kernel's masks stand."""
import json
import multiprocessing as mp
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from helpers import serve_cells as SC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(r):
    return struct.pack("<di", float(r[0]), int(r[1]))


@pytest.fixture(scope="module")
def batches(oracle):
    return SC.generate(oracle)


@pytest.fixture(scope="module")
def want(oracle, batches):
    """{call key: (ee, ns)}: one oracle call per alpha, left unchanged."""
    return SC.expected(oracle, batches)


@pytest.fixture(scope="module")
def calls(batches):
    return SC.calls(batches)


@pytest.fixture(scope="module")
def calls_file(tmp_path_factory, calls, want):
    """The calls and their expectations for the child processes: [[seq, quals, alpha, ee, ns]]."""
    path = str(tmp_path_factory.mktemp("serve") / "calls.json")
    with open(path, "w") as f:
        json.dump([[s, q, a, want[k][0], want[k][1]] for k, s, q, a in calls], f)
    return path


@pytest.fixture(scope="module")
def eng():
    from moira_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def test_in_process_every_read_then_the_sequences(eng, oracle, batches, want, calls):
    """Engine.calculate_errors_PB, one k_serve wave: every generated read in the set's order, then the replay orders (stale bytes
    behind a short read's last chunk; thin and register bodies in turn; the three alphas in turn), three times over."""
    by_key = {k: (s, q, a) for k, s, q, a in calls}
    for k, s, q, a in calls:
        assert bits(eng.calculate_errors_PB(s, q, a)) == bits(want[k]), (k, len(q), a)
    for name, keys in SC.sequences(oracle, batches).items():
        for rnd in range(3):
            for k in keys:
                assert bits(eng.calculate_errors_PB(*by_key[k])) == bits(want[k]), (name, rnd, k)


CHILD = ("import sys, json; sys.path.insert(0, %r)\n"
         "from moira_amd.engine import Engine\n"
         "reads = json.load(open(%r))\n"
         "with Engine(0) as e: print(json.dumps([e.calculate_errors_PB(r[0], r[1], r[2]) for r in reads]))\n")


def test_the_launch_per_call_is_the_oracle_too(calls, want, calls_file):
    """MPB_SERVE=0, in a fresh process: k_small's launch per call (thin bodies only, plain loads) on every read."""
    r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, calls_file)], capture_output=True, text=True, timeout=120, cwd=ROOT,
                       env=dict(os.environ, MPB_SERVE="0"))
    assert r.returncode == 0, r.stderr[-1500:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert len(got) == len(calls)
    for (k, s, q, a), g in zip(calls, got):
        assert bits(g) == bits(want[k]), (k, len(q), a)


@pytest.mark.parametrize("form", ["direct", "copies", "lanes"])
def test_broker_one_client_and_the_solo_count(oracle, batches, want, calls, monkeypatch, form):
    """The broker's three forms (the environment of tests/test_gpu_broker.py) with one client: every read is the oracle's, and
    `solo` -- reads run alone, through the host path -- is exactly what the cells say (mpb_broker.cpp: run_solo is called for a read
    with a private table, for one longer than the form's kernel takes, and for one that came back with pass = 2; with one client
    no lanes micro-batch mixes alphas, so nothing else reaches it).  direct and copies (k_serve): the J = 65 .. 67 reads of the
    register body, the 2048-base reads, the private tables -- and not one of the reads whose prediction is too small, which the
    register body finishes.  lanes (k_small, thin bodies): those under-predicted reads and the J = 65 .. 67 reads miss their cap,
    the 2048-base reads are served.  Where the box refuses direct serving the direct form is the copies form: the same count."""
    from moira_amd import broker
    monkeypatch.setenv("MPB_BROKER_SERVER", "0" if form == "lanes" else "1")
    monkeypatch.setenv("MPB_BROKER_DIRECT", "0" if form == "copies" else "1")
    name = "gpuserve%s_%d" % (form, os.getpid())
    cl = broker.client(0, name=name, idle_exit=5.0)
    try:
        for k, s, q, a in calls:
            assert bits(cl.calculate_errors_PB(s, q, a)) == bits(want[k]), (k, len(q), a)
        st = broker.stats(name)
    finally:
        cl.close()
        broker.shutdown(name)
    expect = SC.solo_expected(oracle, batches, "lanes" if form == "lanes" else "serve")
    assert st["served"] == len(calls) and st["solo"] == expect, (st, expect)


ORDERS = ("forward", "backward", "shuffled")


def _client(name, path, order, out):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    from helpers.broker_slot import DirectSlot
    from moira_amd import broker
    reads = json.load(open(path))
    idx = list(range(len(reads)))
    if order == "backward":
        idx.reverse()
    if order == "shuffled":
        idx = [int(i) for i in np.random.default_rng(7).permutation(len(reads))]
    cl = broker.client(0, name=name, idle_exit=5.0)
    entry = DirectSlot(cl).index
    bad = []
    for i in idx:
        s, q, a, ee, ns = reads[i]
        got = cl.calculate_errors_PB(s, q, a)
        if bits(got) != bits((ee, ns)) and len(bad) < 5:
            bad.append((i, got, (ee, ns)))
    out.put((entry, bad, len(idx)))
    cl.close()


def test_broker_three_clients_on_entries_0_1_2(oracle, batches, calls, calls_file, monkeypatch):
    """Three processes attached at once hold the slots -- the kernel's entries -- 0, 1 and 2; each replays the whole set in an order
    of its own (forward, backward, shuffled).  The only directed input that meets the entry arithmetic at(base, e * step) with
    e > 0.  Each client's reads that are handed back are run alone once each."""
    from moira_amd import broker
    monkeypatch.setenv("MPB_BROKER_SERVER", "1")
    monkeypatch.setenv("MPB_BROKER_DIRECT", "1")
    name = "gpuserve3_%d" % os.getpid()
    ctx = mp.get_context("spawn")
    out = ctx.Queue()
    hold = broker.client(0, name=name, idle_exit=5.0)          # the broker is up before the three start; this slot is given back
    hold.close()
    procs = [ctx.Process(target=_client, args=(name, calls_file, order, out)) for order in ORDERS]
    try:
        for p in procs:
            p.start()
        res = [out.get(timeout=120) for _ in procs]
        for p in procs:
            p.join(30)
        st = broker.stats(name)
    finally:
        broker.shutdown(name)
    assert all(r[1] == [] for r in res), [r[1] for r in res if r[1]]
    assert sorted(r[0] for r in res) == [0, 1, 2]
    assert st["served"] == 3 * len(calls) and st["solo"] == 3 * SC.solo_expected(oracle, batches, "serve"), st


FORGED_LENGTHS = tuple(range(284, 301)) + (1, 15, 16, 17)


def test_a_forged_length_word_sees_only_its_prefix(oracle):
    """Direct serving: the door word of a client-writable slot names a length shorter than the row that lies there -- an honest
    300-base row without a zero byte -- so the bytes from that length to the end of its 16-byte chunk are real scores, not the
    identity step a packed row ends in.  The answer is the oracle's for that prefix: the register body's masks, not the packing,
    keep them out.  (Nothing but the length is forged; the token order is the existing forged-slot test's.)"""
    from helpers.broker_slot import DirectSlot
    from moira_amd import broker
    name = "gpuservelen_%d" % os.getpid()
    cl = broker.client(0, name=name, idle_exit=5.0)
    try:
        rng = np.random.default_rng(11)
        s = "".join("ACGT"[int(v)] for v in rng.integers(0, 4, 300))
        q = [int(v) for v in rng.integers(8, 41, 300)]
        want = oracle.ee_rowwise(s, q, 0.005)
        assert want[2] <= SC.REG_MAX_ROWS
        assert cl.calculate_errors_PB(s, q, 0.005) == want[:2]          # the kernel is up, the slot holds the honest row
        slot = DirectSlot(cl)
        if not slot.served_directly():
            pytest.skip("the broker is not serving the slots directly on this box (registration refused): nothing to forge")
        assert bytes(slot.row[:300]) == bytes(q) and not (slot.row[:304] == 0)[:300].any()
        for n in FORGED_LENGTHS:
            assert 0 < n <= 300
            exp = oracle.ee_rowwise(s[:n], q[:n], 0.005)
            ee, ns, ps = slot.post(n)
            assert ps != 2 and bits((ee, ns)) == bits(exp[:2]), (n, ee, ns, ps, exp)
        assert cl.calculate_errors_PB(s, q, 0.005) == want[:2]          # the client's own next call follows the forged tokens
    finally:
        cl.close()
        broker.shutdown(name)
