"""numpy restatement of MPB_FLAG_ODDS' arithmetic (ODDS_MODE.md; moira_amd/csrc/mpb_dp_tiles.inc with MPB_AR_ODDS), with a
multiply and an addition where the kernel has one fused operation: its rounding error is the kernel's or worse."""
import numpy as np

P0_MIN = 2.0 ** -900            # the range guard: every w[j] <= 1 / p0


def tables():
    """{a, r} per byte code: a = 1 - p, r = p / (1 - p), p = 10^(-q/10); codes 0 ('N') and 255 ('n') are the identity {1, 0}."""
    p = np.array([pow(10, q / -10.0) for q in range(256)])
    with np.errstate(divide="ignore"):                   # code 0 stands for 'N', not for Q0
        a, r = 1 - p, p / (1 - p)
    a[[0, 255]], r[[0, 255]] = 1.0, 0.0
    return a, r


def fused_minus(c, x, y):
    """c - x * y with the product unrounded, as the kernel's fma has it (Veltkamp / Dekker: the product's rounding error is
    recovered exactly and subtracted after the difference)."""
    split = lambda v: ((v * 134217729.0) - ((v * 134217729.0) - v), v - ((v * 134217729.0) - ((v * 134217729.0) - v)))
    p, (xh, xl), (yh, yl) = x * y, split(x), split(y)
    err = ((xh * yh - p) + xh * yl + xl * yh) + xl * yl
    return (c - p) - err


def run(q, lens, alpha, rows):
    """(ee, p0, w): `rows` coefficients w of prod (1 + r_k x) per read, p0 = prod a_k in base order; ee from the CDF of w against
    (1 - alpha) / p0 (NaN: no crossing inside `rows`, or p0 under the guard)."""
    a, r = tables()
    n = len(q)
    live = np.arange(q.shape[1])[None, :] < np.asarray(lens)[:, None]
    w, p0 = np.zeros((n, rows)), np.ones(n)
    w[:, 0] = 1.0
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for k in range(int(np.max(lens))):
            code = np.where(live[:, k], q[:, k], 0)
            w[:, 1:] += r[code][:, None] * w[:, :-1]
            p0 *= a[code]
        thr = (1 - alpha) / p0
        cdf = np.cumsum(w, axis=1)                       # sequential, row 0 first
        above = cdf > thr[:, None]
        j = above.argmax(axis=1)
        hi = cdf[np.arange(n), j]
        lo = np.where(j > 0, cdf[np.arange(n), np.maximum(j - 1, 0)], 0.0)
        # the numerator in the reference's own scale, thr - p0 * lo: a read that crosses in row 1 (lo == 1) then has the
        # reference's fl(thr - P0) bit for bit, where thr / p0 - 1 would have lost every digit of a tiny ee
        ee = np.maximum((j - 1) + fused_minus(1 - alpha, p0, lo) / (p0 * (hi - lo)), 0.0)
    ee[~above.any(axis=1) | ~(p0 >= P0_MIN)] = np.nan
    return ee, p0, w
