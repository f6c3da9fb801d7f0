"""What a batch run with MPB_FLAG_FAST_FMA or MPB_FLAG_ODDS must return, read by read: the CPU model of the mode's arithmetic
(oracle/pb_oracle.c, pbo_filter_batch_model) where the mode keeps the read, the exact oracle where its rules hand the read to
the three-rounding pass.  Equality is bit for bit in ee (NaN equals NaN), identical ns and pass.

Two forms of the rule:
  exact form    (one resident batch through the sorted pipeline, per-read row budgets known): a read is exact when it is in
                the hand-back mask H, when its budget is 0 (k_wide, or settled by decision_only), or when the model needs more
                rows than its budget (the class never crosses: the overflow pass runs it); every other read equals the model.
  counting form (no budgets: host-pipeline chunks, the classified entry): every read equals the model or the exact oracle,
                every read of H equals the exact oracle, and the reads that differ from the model are at most n_overflow plus
                the k_wide reads.
"""
import numpy as np


def same(a, b):
    """Per read: bit for bit (NaN equals NaN)."""
    return (a == b) | (np.isnan(a) & np.isnan(b))


def expect(exact, model, budgets=None):
    """exact: (ee, ns, pass) of the exact oracle; model: pb_oracle.filter_batch_model's result; budgets: per-read row caps
    (Engine.read_budgets) or None.  -> dict(ee, ns, passed, must_exact): each read's expected results, and which reads must
    be exact (H alone when no budgets are given)."""
    ee0, ns0, ps0 = exact
    must = model.hand.copy()
    if budgets is not None:
        budgets = np.asarray(budgets)
        must |= (budgets == 0) | (model.rows > budgets)
    return dict(ee=np.where(must, ee0, model.ee), ns=np.asarray(ns0).copy(),
                passed=np.where(must, np.asarray(ps0).astype(bool), model.passed), must_exact=must)


def differs(exact, model):
    """Reads outside H whose model result (ee, pass) differs from the exact oracle's."""
    ee0, _, ps0 = exact
    return ~model.hand & ~(same(model.ee, ee0) & (model.passed == np.asarray(ps0).astype(bool)))


def matches(got_ee, got_ns, got_pass, ee, ns, passed):
    return same(got_ee, ee) & (np.asarray(got_ns) == ns) & (np.asarray(got_pass).astype(bool) == passed)


def check_exact_form(got, exact, model, budgets, n_overflow, settled=None):
    """got: (ee, ns, pass) from the GPU.  settled (decision_only): reads the prepass settled (+inf, fail); they are left out of
    the rule.  Returns (|H|, budget misses predicted, exact reads that are not k_wide's)."""
    budgets = np.asarray(budgets)
    want = expect(exact, model, budgets)
    ok = matches(*got, want["ee"], want["ns"], want["passed"])
    if settled is not None:
        ok |= settled
    bad = np.flatnonzero(~ok)
    assert bad.size == 0, "%d reads differ from the rule, first %s: got %r want %r (exact %r, hand %r, rows %r, cap %r)" % (
        bad.size, bad[:5].tolist(), got[0][bad[:5]].tolist(), want["ee"][bad[:5]].tolist(), exact[0][bad[:5]].tolist(),
        model.hand[bad[:5]].tolist(), model.rows[bad[:5]].tolist(), budgets[bad[:5]].tolist())
    live = budgets > 0
    misses = live & ~model.hand & (model.rows > budgets)
    to_overflow = live & want["must_exact"]
    assert n_overflow == int(to_overflow.sum()), (n_overflow, int(to_overflow.sum()), int(model.hand.sum()), int(misses.sum()))
    return int(model.hand.sum()), int(misses.sum()), int(to_overflow.sum())


def check_counting_form(got, exact, model, n_overflow, n_wide=0):
    """Returns the number of reads that differ from the model."""
    ee0, ns0, ps0 = exact
    eq_model = matches(*got, model.ee, ns0, model.passed)
    eq_exact = matches(*got, ee0, ns0, np.asarray(ps0).astype(bool))
    bad = np.flatnonzero(~(eq_model | eq_exact))
    assert bad.size == 0, "%d reads equal neither the model nor the exact oracle, first %s" % (bad.size, bad[:5].tolist())
    bad = np.flatnonzero(model.hand & ~eq_exact)
    assert bad.size == 0, "%d reads of H are not exact, first %s" % (bad.size, bad[:5].tolist())
    off_model = int((~eq_model).sum())
    assert off_model <= n_overflow + n_wide, (off_model, n_overflow, n_wide)
    return off_model


def check_mode_ran(got, exact, model, among=None):
    """The share of reads that equal the model and differ from the exact oracle is at least half the share the CPU measures
    (differs()).  among (exact form): the reads the rule leaves to the mode (a batch run with test_underpredict hands most
    of its reads to the exact pass); both shares are taken over them.  Returns (GPU share, CPU share)."""
    ee0, ns0, ps0 = exact
    sel = np.ones(len(ee0), bool) if among is None else among
    k = max(1, int(sel.sum()))
    cpu = float((differs(exact, model) & sel).sum()) / k
    eq_model = matches(*got, model.ee, ns0, model.passed)
    eq_exact = matches(*got, ee0, ns0, np.asarray(ps0).astype(bool))
    gpu = float((eq_model & ~eq_exact & sel).sum()) / k
    assert gpu >= 0.5 * cpu, (gpu, cpu)
    return gpu, cpu
