"""The device tail of --error_calc poisson (k_poisson_tail, include/moira_pb.h "the device tail"): a numpy restatement of its
arithmetic and hand-back rule, the yardstick it is held against (mpb_poisson_finish_host: needs no device), and the input
families the CPU model test and the GPU tests share."""
import ctypes as C
import math

import numpy as np

from moira_amd import _lib as L

WINDOW = 2.0 ** -17            # rule (b): MPB_PT_WINDOW of moira_amd/csrc/mpb_internal.h
LAMBDA_MAX = 64.0              # rule (a): MPB_PT_LAMBDA_MAX
ALPHAS = (1e-5, 1e-4, 0.005, 0.05, 0.5)      # the GPU grid's
MODEL_ALPHAS = ALPHAS + (0.9,)
AMBIGS = ("treat_as_errors", "ignore", "disallow")
CONTRACT = 1e-9
CAP_SHARE = 0.001              # reads rules (b) and (c) may hand back beyond the planted ones, as a share of the batch


def settings(alphas=ALPHAS):
    """The grid of the lambda test: alpha x ambigs x --round x (uncert 0.01 | maxerrors 2.5)."""
    for alpha in alphas:
        for ambigs in AMBIGS:
            for round_ in (False, True):
                for lim in (dict(uncert=0.01), dict(maxerrors=2.5)):
                    yield dict(alpha=alpha, ambigs=ambigs, round_=round_, **lim)


# ---- the yardstick -------------------------------------------------------------------------------------------------------
def host_tail(lams, ns, lens, **kw):
    """mpb_poisson_finish_host -> (ee, pass): pinned to the reference's own results by tests/test_poisson.py."""
    from moira_amd.engine import Engine
    lib = L.load()
    prm = Engine.params(**kw)
    lams = np.ascontiguousarray(lams, np.float64)
    ns = np.ascontiguousarray(ns, np.int32)
    lens = np.ascontiguousarray(lens, np.int32)
    ee = np.empty(len(lams))
    ps = np.empty(len(lams), np.uint8)
    L.check(lib.mpb_poisson_finish_host(lams.ctypes.data, ns.ctypes.data, lens.ctypes.data, 0, len(lams), C.byref(prm),
                                        ee.ctypes.data, ps.ctypes.data))
    return ee, ps


def poisson_ee(lam, alpha):
    """The reference's formula on a given lambda (moira/moira.py:1666-1679), in Python floats; OverflowError as there."""
    lam = float(lam)
    acc, j = [0], 0
    while True:
        acc.append(acc[-1] + (math.exp(-lam) * (lam ** j)) / math.factorial(j))
        if acc[-1] > (1 - alpha):
            break
        j += 1
    e = (j - 1) + ((j - (j - 1)) * ((1 - alpha) - acc[-2]) / (acc[-1] - acc[-2]))
    return 0 if e < 0 else e


def host_cross_term(raw_ee):
    """The term the host's CDF crossed in, from its RAW ee (ambigs ignore, no --round): ee lies in (j - 1, j] for a crossing in
    term j >= 1 (the fraction is positive unless the CDF equals 1 - alpha to the last bit) and is 0 for term 0."""
    return np.where(np.isnan(raw_ee) | (raw_ee == 0), 0, np.ceil(np.nan_to_num(raw_ee))).astype(np.int64)


def close(ee, ps, host_ee, host_ps):
    """Per read: exact (bit for bit, NaN at the same places) or close (|ee - host| <= 1e-9 |host| and pass equal; where either
    side is 0 both are)."""
    ee, host_ee = np.asarray(ee, np.float64), np.asarray(host_ee, np.float64)
    same_pass = np.asarray(ps).astype(np.uint8) == np.asarray(host_ps).astype(np.uint8)
    nan = np.isnan(ee) | np.isnan(host_ee)
    zero = (ee == 0) | (host_ee == 0)
    with np.errstate(invalid="ignore"):
        near = np.abs(ee - host_ee) <= CONTRACT * np.abs(host_ee)
    ok = np.where(nan, np.isnan(ee) & np.isnan(host_ee), np.where(zero, ee == host_ee, near))
    return ok & same_pass


def exact(ee, ps, host_ee, host_ps):
    ee, host_ee = np.asarray(ee, np.float64), np.asarray(host_ee, np.float64)
    return ((ee == host_ee) | (np.isnan(ee) & np.isnan(host_ee))) & (np.asarray(ps).astype(np.uint8) == np.asarray(host_ps).astype(np.uint8))


def rel_err(ee, host_ee):
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.abs(ee - host_ee) / np.abs(host_ee)
    return np.where(host_ee == 0, np.where(ee == 0, 0.0, np.inf), r)


# ---- the model -------------------------------------------------------------------------------------------------------------
def model(lams, ns, lens, ulp=0, alpha=0.005, uncert=0.01, maxerrors=None, ambigs="treat_as_errors", round_=False):
    """k_poisson_tail in numpy, with em = exp(-lambda) moved by `ulp` units in the last place (the device's exp is not the
    host's).  -> dict: ee / ps of the reads it keeps (ee = lambda, ps = 2 where handed back), back = a | b | c, j = the
    crossing term (-1 where rule (a) applies)."""
    lam = np.asarray(lams, np.float64)
    ns = np.asarray(ns, np.int64)
    li = np.asarray(lens, np.int64)
    n = len(lam)
    thr = 1 - alpha
    with np.errstate(invalid="ignore"):
        a = ~((lam >= 0.0) & (lam <= LAMBDA_MAX))
    l0 = np.where(a, 0.0, lam)
    em = np.exp(-l0)
    for _ in range(abs(ulp)):
        em = np.nextafter(em, np.inf if ulp > 0 else -np.inf)
    t, acc_prev, acc = em.copy(), np.zeros(n), em.copy()
    j = np.zeros(n, np.int64)
    for step in range(1, 171):
        live = ~(acc > thr)
        if not live.any():
            break
        t_new = (t * l0) / float(step)
        acc_new = acc + t_new
        j = np.where(live, step, j)
        t = np.where(live, t_new, t)
        acc_prev = np.where(live, acc, acc_prev)
        acc = np.where(live, acc_new, acc)
    uncrossed = ~(acc > thr)
    b = ~a & ~uncrossed & (j <= 1) & (np.abs(thr - em) < WINDOW)
    with np.errstate(invalid="ignore", divide="ignore"):
        e = (j - 1).astype(np.float64) + (thr - acc_prev) / (acc - acc_prev)
    e = np.where(e < 0, 0.0, e)
    if ambigs == "treat_as_errors":
        e = e + ns.astype(np.float64)
    limit = np.full(n, float(maxerrors)) if maxerrors is not None else li.astype(np.float64) * uncert
    with np.errstate(invalid="ignore"):
        tol = 1e-9 * np.maximum(1.0, np.abs(e))
        unsure = np.abs(e - limit) <= tol
        if round_:
            unsure |= np.abs(e - np.rint(e)) <= tol
    c = ~a & ~uncrossed & ~b & (j > 0) & unsure
    back = a | uncrossed | b | c
    if round_:
        e = np.floor(e)
    with np.errstate(invalid="ignore"):
        keep = e <= limit
    if ambigs == "disallow":
        keep &= ~(ns > 0)
    return dict(ee=np.where(back, lam, e), ps=np.where(back, 2, keep).astype(np.uint8), back=back, a=a, b=b, c=c,
                j=np.where(a, -1, j))


# ---- input families ------------------------------------------------------------------------------------------------------------
GRID_N = 4099


def lambda_grid(alpha, seed=11):
    """The lambda grid of the GPU test for one alpha -> dict(lam, ns, lens (ragged 50..600), n_range = reads of rule (a),
    n_planted = the crossing point exp(-lambda) == 1 - alpha and its forty neighbours)."""
    rng = np.random.default_rng(seed)
    l0 = -math.log(1 - alpha)
    d = np.geomspace(np.spacing(l0), 2 * WINDOW, 20)
    planted = np.concatenate([[l0], l0 - d, l0 + d])
    beyond = rng.uniform(64, 200, 300)
    parts = [[0.0, 1e-300, 1e-9], planted, rng.uniform(0, 8, 2000), rng.uniform(8, 64, 1500), rng.uniform(0, 0.1, 250),
             [64.0, np.nextafter(64.0, 65.0)], beyond, [np.nan, np.inf, -1.0]]
    lam = np.concatenate([np.asarray(p, np.float64) for p in parts])
    assert len(lam) == GRID_N
    lam = lam[rng.permutation(GRID_N)]
    with np.errstate(invalid="ignore"):
        n_range = int((~((lam >= 0) & (lam <= LAMBDA_MAX))).sum())
    return dict(lam=lam, ns=rng.integers(0, 4, GRID_N).astype(np.int32), lens=rng.integers(50, 601, GRID_N).astype(np.int32),
                n_range=n_range, n_planted=len(planted))


def limit_family(seed=12):
    """Decisions on the limit: 1,000 lambda uniform in (0, 20), fixed length 300."""
    rng = np.random.default_rng(seed)
    n = 1000
    return dict(lam=rng.uniform(0, 20, n), ns=rng.integers(0, 4, n).astype(np.int32), lens=np.full(n, 300, np.int32))


def integer_lambdas(alpha=0.005, targets=(1, 2, 3, 4, 5, 6)):
    """lambda whose ee (the Python formula) lies within 1e-10 of an integer: bisection on the formula, which grows with lambda."""
    out = []
    for m in targets:
        lo, hi = 0.0, 40.0
        while True:
            mid = 0.5 * (lo + hi)
            if mid <= lo or mid >= hi:
                break
            if poisson_ee(mid, alpha) < m:
                lo = mid
            else:
                hi = mid
        best = min((lo, hi), key=lambda x: abs(poisson_ee(x, alpha) - m))
        assert abs(poisson_ee(best, alpha) - m) <= 1e-10, (m, best)
        out.append(best)
    return np.array(out)


MATRIX_STRIDES = (16, 320, 608)


def matrix_family(stride, seed=None, n=1000):
    """A ragged matrix (lengths 0..stride, garbage -- bytes 0 and 255 included -- in the padding, 3 % 'N') and its fixed-length
    twin (every row read in full: no byte 255 left) -> (q, lens, q_full)."""
    rng = np.random.default_rng(stride if seed is None else seed)
    lens = rng.integers(0, stride + 1, n).astype(np.int32)
    lens[:3] = (0, 1, stride)
    q = rng.integers(1, 60, (n, stride)).astype(np.uint8)
    q[rng.random((n, stride)) < 0.03] = 0
    pad = np.arange(stride)[None, :] >= lens[:, None]
    q[pad] = rng.integers(0, 256, int(pad.sum()), dtype=np.uint8)
    full = q.copy()
    full[full == 255] = 17
    return q, lens, full


def handed_back_family():
    """Everything handed back: 300 reads of 1,024 bases at Q10 (lambda = 102.4: finite on the host) and 300 of 2,048 bases at Q3
    (NaN on the host) -> [(q, fixed_len)]."""
    return [(np.full((300, 1024), 10, np.uint8), 1024), (np.full((300, 2048), 3, np.uint8), 2048)]


def lambda_of(q, lens=None, chunk=20000):
    """lambda / Ns of a packed matrix as k_lambda computes them: the sum of 10 ** (Q / -10) over the non-'N' bases IN BASE ORDER."""
    p = np.array([0.0] + [10 ** (v / -10.0) for v in range(1, 256)])
    n, stride = q.shape
    lens = np.full(n, stride, np.int64) if lens is None else np.asarray(lens, np.int64)
    lam, ns = np.zeros(n), np.zeros(n, np.int32)
    col = np.arange(stride)[None, :]
    for lo in range(0, n, chunk):
        blk = q[lo:lo + chunk]
        inside = col < lens[lo:lo + chunk, None]
        run = np.cumsum(np.where(inside, p[blk], 0.0), axis=1)          # x + 0.0 == x: the sequential sum of the read's bases
        lam[lo:lo + chunk] = run[:, -1]
        ns[lo:lo + chunk] = ((blk == 0) & inside).sum(1)
    return lam, ns
