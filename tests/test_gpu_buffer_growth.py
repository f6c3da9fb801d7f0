"""Every block of a context created, carved and regrown in one run, with the per-read entry's resident server (k_serve) alive in
between: the host layer keeps each block behind one owner (moira_amd/csrc/mpb_ctx.h: Buf, Carver), which asks the server to leave
before it frees anything.  One fresh context, so that every block starts at zero capacity; every result is the oracle's bit for
bit (the Poisson step: mpb_poisson_finish_host under the device tail's contract, as tests/test_gpu_poisson_device.py)."""
import numpy as np
import pytest

from helpers import poisson_tail_model as P

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def resident(eng, q, lens, **kw):
    """A host matrix + lengths through mpb_filter_device -> (ee, ns, pass, counts); the caller's buffers are freed before the
    queries that follow (mpb_free asks the server to leave as well)."""
    n, stride = q.shape
    bufs = [eng.alloc(n * stride).upload(np.ascontiguousarray(q)), eng.alloc(n * 4).upload(np.ascontiguousarray(lens, np.int32)),
            eng.alloc(n * 8).upload(np.full(n, -7.0)), eng.alloc(n * 4).upload(np.full(n, -7, np.int32)),
            eng.alloc(n).upload(np.full(n, 9, np.uint8))]
    d_q, d_len, d_ee, d_ns, d_pass = bufs
    try:
        c = eng.filter_device(d_q, n, stride, d_len=d_len, d_ee=d_ee, d_ns=d_ns, d_pass=d_pass, params=eng.params(**kw))
        return d_ee.download(np.float64, n), d_ns.download(np.int32, n), d_pass.download(np.uint8, n), c
    finally:
        for b in bufs:
            b.free()


def test_every_block_grows_with_the_server_alive(oracle):
    from moira_amd.engine import Engine
    rng = np.random.default_rng(41)
    read = ("ACGNT" * 20, [int(v) for v in rng.integers(2, 41, 100)], 0.005)            # 100 bases: the server's
    want_read = oracle.ee_rowwise(*read)[:2]

    def batch(n, stride, lo, hi, seed, profile=0):
        q, lens = oracle.synth_fill(n, stride, min_len=lo, max_len=hi, seed=seed, profile=profile)
        return q, lens, oracle.filter_batch(q, lens=lens, threads=8)

    def host_fed(eng, b, n=None):
        q, lens, (ee, ns, ps, _) = b
        n = len(lens) if n is None else n
        r = eng.filter(q[:n], lens=lens[:n])
        assert np.array_equal(bits(r.ee), bits(ee[:n])) and np.array_equal(r.ns, ns[:n]) and np.array_equal(r.passed, ps[:n] != 0)
        assert r.n_pass == int(ps[:n].sum())
        return r

    small, piped = batch(64, 48, 1, 48, 2), batch(5000, 48, 1, 48, 4)
    eng = Engine(0)
    try:
        assert eng.calculate_errors_PB(*read) == want_read              # 1: the resident server starts
        host_fed(eng, small)                                            # 2: the small path: stage + pinned block (the server leaves first)
        assert eng.calculate_errors_PB(*read) == want_read              # 3: ... and is launched again
        host_fed(eng, piped)                                            # 4: the pipeline: slots and the sorted pipeline's workspace
        assert eng.calculate_errors_PB(*read) == want_read              # 5
        # 6: resident, rows that can hold more than 1023 bases (one read does): the wide list
        q, lens, (ee, ns, ps, _) = batch(3000, 1040, 50, 600, 6)
        q[17, :1030] = rng.integers(2, 41, 1030, dtype=np.uint8)
        lens[17] = 1030
        ee, ns, ps, _ = oracle.filter_batch(q, lens=lens, threads=8)
        e1, n1, p1, c = resident(eng, q, lens)
        assert np.array_equal(bits(e1), bits(ee)) and np.array_equal(n1, ns) and np.array_equal(p1, ps) and c.n_pass == int(ps.sum())
        hist = eng.class_histogram()                                    # (a fetch into the caller's frame)
        assert 3000 - 1 <= sum(hist.values()) <= 3000                   # every read in a class, but read 17 if it ran wide
        # 7: the narrow pass forced with three rows on ragged batches: both of its blocks, created and then regrown
        for n in (9000, 20000):
            q, lens, (ee, ns, ps, _) = batch(n, 64, 1, 64, 7, profile=1)
            e1, n1, p1, c = resident(eng, q, lens, narrow_rows=3)
            assert eng.last_path()["narrow_rows"] == 3
            assert np.array_equal(bits(e1), bits(ee)) and np.array_equal(n1, ns) and np.array_equal(p1, ps) and c.n_pass == int(ps.sum())
        assert eng.calculate_errors_PB(*read) == want_read              # 8
        # 9: the resident Poisson filter: the record block of the device tail
        q, lens, _ = P.matrix_family(320, n=3000)
        n = len(lens)
        d_q, d_len = eng.alloc(q.nbytes).upload(np.ascontiguousarray(q)), eng.alloc(n * 4).upload(np.ascontiguousarray(lens, np.int32))
        d_ee, d_ns, d_pass, d_lam = eng.alloc(n * 8), eng.alloc(n * 4), eng.alloc(n), eng.alloc(n * 8)
        try:
            c = eng.filter_poisson_device(d_q, n, 320, d_len=d_len, d_ee=d_ee, d_ns=d_ns, d_pass=d_pass, d_lambda=d_lam,
                                          params=eng.params(alpha=0.005))
            lam, ns = d_lam.download(np.float64, n), d_ns.download(np.int32, n)
            ee, ps = d_ee.download(np.float64, n), d_pass.download(np.uint8, n)
        finally:
            for b in (d_q, d_len, d_ee, d_ns, d_pass, d_lam):
                b.free()
        want_lam, want_ns = P.lambda_of(q, lens)
        # (lambda: a sum of at most 320 positive terms in base order -- 320 roundings of 2^-53 bound any difference in the terms'
        # last bits by 4e-14 relative; a wrong pointer gives garbage, not that)
        assert np.allclose(lam, want_lam, rtol=4e-14, atol=0) and np.array_equal(ns, want_ns)
        want_ee, want_ps = P.host_tail(lam, ns, lens, alpha=0.005)
        assert P.close(ee, ps, want_ee, want_ps).all() and c.n_reads == n and c.n_pass == int(ps.sum())
        # 10: the host-fed paths again with fewer reads (nothing regrows): the bits of a fresh run of those inputs
        host_fed(eng, small, 40)
        host_fed(eng, piped, 4500)
    finally:
        eng.close()                                                     # 11
    with Engine(0) as eng:
        assert eng.calculate_errors_PB(*read) == want_read
