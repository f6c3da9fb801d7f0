"""The rule for MPB_FLAG_ODDS | MPB_FLAG_ODDS_NARROW with a forced row count R, shared by tests/test_gpu_odds_narrow.py and
tests/test_gpu_narrow_walk.py: with F = ~m.hand & ~has_255 & (m.rows <= R) (and the length valid), every read of F equals the model
bit for bit, last_path() says narrow_rows == R and n_fallback == n - |F|, all reads satisfy the counting form
(tests/helpers/mode_expect.py) and the mode is seen to have run over F."""
import numpy as np

from helpers import mode_expect as X
from helpers import odds_narrow_inputs as N
from helpers.device_runs import Resident


def run(eng, q, lens, fixed, **kw):
    """One resident batch through mpb_filter_device -> ((ee, ns, pass), counts, path)."""
    res = Resident(eng, q, None if fixed else lens)
    try:
        ee, ns, ps, c, path, intact = res.run(fixed_len=fixed, **kw)
        assert intact
        return (ee, ns, ps), c, path
    finally:
        res.free()


def check_forced_results(got, c, path, q, lens, R, ex, m, valid=None, mode_ran=True):
    """The rule on the results of one run (got = (ee, ns, pass), c its counts, path its last_path()) -> (|F|, n_overflow)."""
    n = len(q)
    F = N.finished(m, q, lens, R)
    if valid is not None:
        F &= valid
    assert path["narrow_rows"] == R and path["narrow_split"] == 0, path
    ok = X.matches(*got, m.ee, ex[1], m.passed)
    bad = np.flatnonzero(F & ~ok)
    assert bad.size == 0, "%d reads the pass finishes differ from the model, first %s: got %r want %r (exact %r)" % (
        bad.size, bad[:5].tolist(), got[0][bad[:5]].tolist(), m.ee[bad[:5]].tolist(), ex[0][bad[:5]].tolist())
    assert path["n_fallback"] == n - int(F.sum()), (path["n_fallback"], n - int(F.sum()))
    X.check_counting_form(got, ex, m, c.n_overflow)
    if mode_ran:
        X.check_mode_ran(got, ex, m, among=F)
    return int(F.sum()), c.n_overflow


def check_forced(eng, q, lens, fixed, R, ex, m, valid=None, mode_ran=True, **kw):
    """One forced run and the rule -> (|F|, n_overflow)."""
    got, c, path = run(eng, q, lens, fixed, odds=True, odds_narrow=True, narrow_rows=R, **kw)
    return check_forced_results(got, c, path, q, lens, R, ex, m, valid=valid, mode_ran=mode_ran)
