"""The inputs of tests/test_gpu_odds_narrow.py, shared with tests/test_odds_narrow_inputs.py (which checks on the CPU that they
exercise every row count of the one-FMA narrow pass and lie within the 1e-9 contract, so that a GPU failure is the kernel's).

One batch per shape (L, stride, ragged): n = 1000 + L % 7 reads whose scores are drawn around the score at which a read of its
length crosses 1 - alpha in row 1, so that every forced row count R = 2, 3, 4 finishes a good share of the reads AND a good share
cross in the last row the pass keeps; a fifth are bad reads, which no R finishes."""
import functools

import numpy as np

FIXED_SHAPES = [(1, 16), (3, 16), (15, 16), (16, 16), (17, 32), (63, 64), (64, 64), (65, 80), (100, 112), (127, 128), (128, 128),
                (129, 144), (299, 304), (300, 304), (301, 304), (300, 320), (320, 320), (600, 608), (1023, 1024), (1500, 1536),
                (10, 320), (130, 320), (257, 320), (65, 128), (191, 192), (200, 384), (440, 448), (2000, 2048), (30, 1024)]
RAGGED_SHAPES = [(16, 16), (100, 112), (300, 320), (600, 608), (600, 640), (1000, 1024), (4096, 4096)]
ROWS = (2, 3, 4)
PARTIAL_N = (1, 2, 63, 64, 65, 255, 256, 257, 4097)
MODE_KW = [dict(ambigs="treat_as_errors"), dict(ambigs="ignore"), dict(ambigs="disallow"), dict(round_=True),
           dict(ambigs="ignore", maxerrors=0.4), dict(alpha=0.05, uncert=0.002), dict(alpha=0.3), dict(alpha=0.9),
           dict(alpha=1e-4), dict(alpha=1e-5)]
MODE_STRIDES = (320, 304)
THREADS = 16


def batch(L, stride, ragged):
    """-> (q, lens): the shape's batch.  lens is the per-read length of a ragged batch, L everywhere otherwise."""
    rng = np.random.default_rng(1_000_003 * L + 7 * stride + (1 if ragged else 0))
    n = 1000 + L % 7
    if ragged:
        lens = rng.integers(0, L + 1, n).astype(np.int32)
        lens[:4] = (0, L, 1, min(L, 16))
    else:
        lens = np.full(n, L, np.int32)
    qlo = np.clip(np.ceil(10.0 * np.log10(np.maximum(lens, 1) / 0.05)), 20, 60).astype(np.int64)
    role = rng.permutation(n) % 5                          # 0, 1: cross in row 1; 2: row 2; 3: row 3; 4: a bad read
    lo = np.where(role <= 1, qlo, np.where(role == 2, qlo - 10, np.where(role == 3, qlo - 13, 2)))
    hi = np.where(role <= 1, qlo + 8, np.where(role == 2, qlo - 4, np.where(role == 3, qlo - 8, 41)))
    q = (lo[:, None] + np.floor(rng.random((n, stride)) * (hi - lo)[:, None]).astype(np.int64)).astype(np.uint8)
    col = np.arange(stride)[None, :]
    pad = col >= lens[:, None]
    q[pad] = rng.integers(0, 256, int(pad.sum()), dtype=np.uint8)          # anything past a read's end
    for share, byte in ((0.10, 0), (0.05, 255)):
        for i in np.flatnonzero((rng.random(n) < share) & (lens > 0)):
            q[i, rng.integers(0, lens[i])] = byte
    return q, lens


def has_255(q, lens):
    return ((q == 255) & (np.arange(q.shape[1])[None, :] < np.asarray(lens)[:, None])).any(axis=1)


def where(lens, L, ragged):
    return dict(lens=lens) if ragged else dict(fixed_len=L)


@functools.lru_cache(maxsize=None)
def reference(oracle, L, stride, ragged):
    """-> (q, lens, exact (ee, ns, pass), model): computed once per shape, shared and never changed."""
    q, lens = batch(L, stride, ragged)
    w = where(lens, L, ragged)
    ex = oracle.filter_batch(q, threads=THREADS, **w)
    m = oracle.filter_batch_model(q, "odds", threads=THREADS, **w)
    for a in (q, lens) + tuple(ex):
        a.setflags(write=False)
    return q, lens, ex[:3], m, ex[3]


def finished(m, q, lens, R):
    """F: the reads a pass forced to R rows must finish itself (lengths are valid in every batch built here)."""
    return ~m.hand & ~has_255(q, lens) & (m.rows <= R)


def modes_batch(oracle, stride):
    q, lens = oracle.synth_fill(20000, stride, fixed_len=300, seed=5, profile=1)
    q[::7, 5] = 0
    q[::11, 17] = 255
    return q, lens, 300
