"""MPB_FLAG_ODDS_NARROW without a GPU: the inputs of tests/test_gpu_odds_narrow.py exercise every row count of the one-FMA narrow
pass and lie within the contract; the flag's value and its Python surface; the compiled twins' names, registers and instruction
mix (ODDS_MODE.md "The narrow passes")."""
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from helpers import mode_expect as X
from helpers import odds_narrow_inputs as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL_TOL = 1e-9 / 30          # the contract's 1e-9 with a factor of 30 to spare (ODDS_MODE.md: worst seen 3.9e-14)

SHAPES = [(L, s, False) for L, s in N.FIXED_SHAPES] + [(L, s, True) for L, s in N.RAGGED_SHAPES]


@pytest.mark.parametrize("L,stride,ragged", SHAPES)
def test_every_shape_exercises_every_row_count_within_the_contract(oracle, L, stride, ragged):
    q, lens, ex, m, need = N.reference(oracle, L, stride, ragged)
    n = len(q)
    assert n == 1000 + L % 7
    assert int(need.max()) <= 1024                                       # no k_wide
    for R in N.ROWS:
        F = N.finished(m, q, lens, R)
        assert F.sum() >= 0.30 * n, (R, int(F.sum()))
        if L >= 16:
            assert (F & (m.rows == R)).sum() >= 0.10 * n, (R, int((F & (m.rows == R)).sum()))
    out = ~m.hand
    ee0, ns0, ps0 = ex
    assert np.array_equal(m.passed[out], np.asarray(ps0).astype(bool)[out])
    assert np.array_equal(np.isnan(m.ee[out]), np.isnan(ee0[out]))
    fin = out & np.isfinite(ee0) & (ee0 > 0)
    assert np.all(m.ee[out & (ee0 == 0)] == 0)
    worst = float((np.abs(m.ee[fin] - ee0[fin]) / ee0[fin]).max()) if fin.any() else 0.0
    assert worst <= MODEL_TOL, worst
    if not ragged:
        assert not m.hand.any()
    else:
        assert 1 <= int(m.hand.sum()) <= 64 and m.hand[0]                # the empty reads: ee = 0 sits on a limit of 0
        assert (lens[m.hand] == 0).all()
    if L >= 16:
        assert X.differs(ex, m).sum() >= 0.5 * n                         # the model's bits are not the oracle's: equality shows the mode


@pytest.mark.parametrize("stride", N.MODE_STRIDES)
def test_the_modes_batch_within_the_contract(oracle, stride):
    q, lens, fixed = N.modes_batch(oracle, stride)
    for kw in N.MODE_KW:
        ee0, ns0, ps0, need = oracle.filter_batch(q, fixed_len=fixed, threads=N.THREADS, **kw)
        m = oracle.filter_batch_model(q, "odds", fixed_len=fixed, threads=N.THREADS, **kw)
        out = ~m.hand
        assert np.array_equal(m.passed[out], ps0.astype(bool)[out]), kw
        fin = out & np.isfinite(ee0) & (ee0 > 0)
        assert (np.abs(m.ee[fin] - ee0[fin]) / ee0[fin]).max() <= MODEL_TOL, kw
        share = [float(N.finished(m, q, lens, R).mean()) for R in N.ROWS]
        print(kw, "finished at R = 2, 3, 4: %.2f %.2f %.2f" % tuple(share))
        if kw.get("alpha") == 1e-4:
            assert share[0] == 0 and share[1] >= 0.5
        if kw.get("alpha") == 1e-5:
            assert share[0] == 0 and share[1] == 0 and share[2] > 0


def test_flag_value_and_engine_params():
    from moira_amd import _lib as L
    from moira_amd.engine import Engine
    hdr = open(os.path.join(ROOT, "include", "moira_pb.h")).read()
    assert re.search(r"#define MPB_FLAG_ODDS_NARROW\s+\(1u << 20\)", hdr)
    assert L.FLAG_ODDS_NARROW == 1 << 20
    assert L.FLAG_ODDS_NARROW & (L.FLAG_NARROW_ROWS(15) | (255 << 12)) == 0
    f = Engine.params(odds=True, odds_narrow=True).flags
    assert f & L.FLAG_ODDS and f & L.FLAG_ODDS_NARROW
    assert not Engine.params(odds=True).flags & L.FLAG_ODDS_NARROW
    assert Engine.params(odds=True, odds_narrow=True, narrow_rows=3).flags & L.FLAG_NARROW_ROWS(3)
    with pytest.raises(ValueError, match="odds_narrow needs odds"):
        Engine.params(odds_narrow=True)


@pytest.fixture(scope="module")
def isa():
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "k.s")
        subprocess.check_call([hipcc, "-O3", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
                               "-x", "hip", "--cuda-device-only", "-S", "-o", out,
                               os.path.join(ROOT, "moira_amd", "csrc", "mpb_kernels.hip")], stderr=subprocess.DEVNULL)
        text = open(out).read()
    body = {m.group(1): m.group(2) for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M)}
    vgpr = {m.group(1): int(m.group(2)) for m in re.finditer(
        r"\.amdhsa_kernel (\S+)\n(?:.*\n)*?\s*\.amdhsa_next_free_vgpr (\d+)", text)}
    return body, vgpr


# (odds twin, exact twin, R) by mangled-name pattern
TWINS = [(r"10k_odds_narILi%dELi\d+EE", r"8k_narrowILi%dELi\d+EE", R) for R in (2, 3, 4)] + \
        [(r"13k_odds_nar_rsILi%dELb1EE", r"11k_narrow_rsILi%dELb1EE", R) for R in (2, 3, 4)] + \
        [(r"13k_odds_nar_rsILi%dELb0EE", r"11k_narrow_rsILi%dELb0EE", 2)] + \
        [(r"13k_odds_nar_rgILi%dEE", r"11k_narrow_rgILi%dELi%dEE", R) for R in (2, 3, 4)]


def test_the_twins_are_kernels_of_their_own_with_fewer_operations_and_no_more_registers(isa):
    body, vgpr = isa
    count = lambda b: sum(b.count(op) for op in ("v_mul_f64", "v_add_f64", "v_fma_f64", "v_fmac_f64"))
    assert len([k for k in vgpr if "k_odds_nar" in k]) == 10
    for odds_pat, exact_pat, R in TWINS:
        o = [k for k in vgpr if re.search(odds_pat % R, k)]
        e = [k for k in vgpr if re.search(exact_pat % ((R, R) if exact_pat.count("%d") == 2 else R), k)]
        assert len(o) == 1 and len(e) == 1, (odds_pat, R, o, e)
        o, e = o[0], e[0]
        assert "k_narrow" not in o
        assert vgpr[o] <= vgpr[e] and vgpr[o] <= 128, (o, vgpr[o], vgpr[e])
        if "_rg" not in o:
            assert "scratch_" not in body[o], o
        # the base loop is R operations against 3 R - 2; the bound leaves the epilogue (one more division, the guard) room
        assert count(body[o]) < (R + 1) / (3 * R - 2) * count(body[e]), (o, count(body[o]), count(body[e]))
        assert body[o].count("v_fma_f64") + body[o].count("v_fmac_f64") > 0
