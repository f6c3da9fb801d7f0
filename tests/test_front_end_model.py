"""tests/helpers/front_end_model.py without a GPU: the conditions the GPU tests of the front end rely on -- at most 5 % of any batch
inside the band, the float32 model of class_cells.py inside it too, every required shape generated -- and the numpy statement of
the decode rules against the host packer."""
import numpy as np
import pytest

from helpers import class_cells as CC
from helpers import front_end_model as FM


@pytest.fixture(scope="module")
def batches():
    return FM.front_end_batches()


def _models(b):
    return [FM.Model(b.q, b.lens, b.alpha, under) for under in (False, True)]


def test_at_most_five_percent_of_a_batch_is_unsure_and_the_float_model_agrees_on_the_rest(batches):
    """Both are conditions on the inputs: the band may hide at most UNSURE_MAX of a batch (plain and with the halved budgets of
    MPB_FLAG_TEST_UNDERPREDICT), and on a sure read the float32 numpy model gives the float64 budget."""
    for b in batches:
        for under, m in zip((False, True), _models(b)):
            assert m.unsure_share <= FM.UNSURE_MAX, (b.name, under, m.unsure_share)
            f32 = CC.cap_of_rows(CC.predicted_rows(b.q, b.lens, b.alpha, under))
            assert np.array_equal(f32[m.sure], m.budget[m.sure]), (b.name, under)
            assert np.isin(m.budget, np.r_[-1, 0, CC.CAPS]).all()


@pytest.mark.parametrize("family", sorted(FM.FAMILIES))
def test_the_families_at_their_own_stride(family):
    """4,000 reads of each family at every alpha: the unsure share, and float32 against float64 on the sure reads."""
    for k, alpha in enumerate(FM.ALPHAS):
        b = FM.family_batch(family, 4000, alpha, seed=k)
        m = FM.Model(b.q, b.lens, alpha)
        assert m.unsure_share <= FM.UNSURE_MAX, (family, alpha, m.unsure_share)
        f32 = CC.cap_of_rows(CC.predicted_rows(b.q, b.lens, alpha))
        assert np.array_equal(f32[m.sure], m.budget[m.sure]), (family, alpha)
    if family == "wide":
        assert (m.budget == 0).mean() > 0.2
    if family in ("good", "short16"):
        assert (m.budget > 0).all() or (m.budget[m.sure] > 0).all()


def test_the_band_and_the_clamps_by_hand():
    """One read of 40 bases of Q10 at alpha 0.005, worked out here: mu = 4, var = 3.6, k3 = 2.88, z = 2.5758."""
    q = np.full((3, 48), 10, np.uint8)
    lens = np.array([40, 3, 0], np.int32)
    x, scored = FM.x64(q, lens, 0.005)
    z = CC.inv_norm_cdf(0.995)
    assert abs(x[0] - (4 + z * 3.6 ** 0.5 + 0.8 * (z * z - 1) / 6)) < 1e-12 and list(scored) == [40, 3, 0]
    assert list(FM.rows_of(x, scored)) == [int(np.floor(x[0] + 0.5)) + 1, 3, 1]            # 3 bases: at most 4 rows; none: 1
    assert list(FM.rows_of(x, scored, True)) == [(int(np.floor(x[0] + 0.5)) + 1) // 2, 1, 1]
    m = FM.Model(q, lens, 0.005)
    assert list(m.budget) == [12, 3, 2] and m.sure.all()                                    # x = 9.64: 11 rows, cap 12
    # a read on a class edge is unsure, and bracketed: x + 0.5 within the band of an integer whose two sides are two classes
    for xv, sure in ((11.4, True), (11.495, False), (11.52, True)):
        xs = np.array([xv])
        b = FM.BAND_ABS + FM.BAND_REL * xs
        lo, hi = CC.cap_of_rows(FM.rows_of(xs - b, np.array([100]))), CC.cap_of_rows(FM.rows_of(xs + b, np.array([100])))
        assert (lo[0] == hi[0]) == sure and (lo[0], hi[0]) in ((12, 12), (12, 14), (14, 14))
    # the tile / wide edge: 1024 rows is the last tile class, 1025 is wide (budget 0)
    assert list(CC.cap_of_rows(FM.rows_of(np.array([1022.6, 1023.6]), np.array([5000, 5000])))) == [1024, 0]


def test_overflow_bracket():
    m = FM.Model.__new__(FM.Model)
    m.sure = np.array([True, True, True, False, True])
    m.budget = np.array([4, 4, 0, -1, 16], np.int32)
    assert FM.overflow_bracket(m, np.array([5, 4, 2000, 3, 17])) == (2, 4)                   # two misses; one wide, one unsure
    assert FM.overflow_bracket(m, np.array([5, 4, 2000, 3, 17]), among=np.array([1, 1, 0, 0, 0], bool)) == (1, 1)


def test_every_required_shape_is_generated(batches):
    by_name = {b.name: b for b in batches}
    assert len(by_name) == len(batches)
    for n in FM.N_SWEEP:
        f, r = by_name["n%d_fixed40" % n], by_name["n%d_ragged" % n]
        assert (f.n, f.stride, f.fixed_len) == (n, 48, 40) and (r.n, r.stride, r.fixed_len) == (n, 48, None)
        assert r.lens.min() >= 0 and r.lens.max() <= 48
    assert set(FM.N_SWEEP) >= {1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049}
    for n in (262144, 262145):                                     # 256 and 257 blocks of 1024 reads
        assert by_name["scan%d_ragged" % n].n == by_name["scan%d_fixed32" % n].n == n and -(-n // 1024) in (256, 257)
        assert by_name["scan%d_ragged" % n].q.nbytes <= 8 << 20 | 32
    assert sorted(FM.SWEEP) == [16, 64, 320, 944, 960, 976, 1024, 1936, 2048, 4096]
    for stride in FM.SWEEP:
        r = by_name["s%d_ragged" % stride]
        assert (r.n, r.stride) == (1100, stride)
        groups = np.delete(r.lens[:1088].reshape(-1, 16), 1, 0)                          # (group 1: sixteen equal lengths)
        assert (groups == 0).any(1).all() and (groups == stride).any(1).all()            # every group: an empty and a full row
        for res in (15, 0, 1):                                                            # ... and 16 k - 1, 16 k, 16 k + 1
            assert ((groups % 16 == res) & (groups > 0)).any(1).all() or stride == 16
        assert len(set(r.lens[16:32])) == 1 and r.n % 16 != 0                             # equal lengths; a group that straddles n
        for cut in (0, 1, 15, 16):
            assert by_name["s%d_fixed%d" % (stride, stride - cut)].fixed_len == stride - cut
    # the LONG instance of k_prepass switches on above 960 bytes; the marker rows lie on both sides of one and two panels
    assert FM.MARKER_STRIDES == (960, 976, 1920, 1936)
    for stride in FM.MARKER_STRIDES:
        b = by_name["markers%d" % stride]
        seen = {(kind, L) for _, kind, L in b.kinds}
        assert {k for k, _ in seen} == set(FM.MARKER_KINDS) and {L for _, L in seen} >= {stride, stride - 1, stride - 16, 960, 481}
        for i, kind, L in b.kinds:
            row = b.q[i, :L]
            scored = int(((row != 0) & (row != 255)).sum())
            assert b.lens[i] == L and scored == {"all_N": 0, "all_n": 0, "N_n_alternating": 0, "N_then_n": 0, "scored_first_n": 1,
                                                 "scored_last_n": 1}.get(kind, (L - 1) % 16 + 1), (kind, L)
            if kind == "scored_first_n":
                assert row[0] not in (0, 255)
            if kind == "scored_last_n":
                assert row[L - 1] not in (0, 255)
    # k_classify_linear: tile_rows = 1280 / cpr, lanes per row, at every value named
    assert {s: FM.linear_geometry(s) for s in FM.LINEAR_GEOMETRY} == FM.LINEAR_GEOMETRY
    assert [FM.linear_geometry(s)[0] for s in (32, 48, 80, 1264, 1280, 1296, 10240, 10256, 16384)] == [640, 426, 256, 16, 16, 15, 2, 1, 1]
    assert [s // 16 for s in FM.LINEAR_GEOMETRY] == [2, 3, 5, 79, 80, 81, 640, 641, 1024]
    for stride in FM.LINEAR_GEOMETRY:
        r = by_name["s%d_ragged" % stride]
        if stride >= 10240:
            wide = FM.Model(r.q, r.lens, r.alpha).budget == 0
            assert r.n == 40 and wide.sum() == 1 and wide[7]
        else:
            assert r.n == max(1100, 2 * FM.linear_geometry(stride)[0] + 3) and r.n % FM.linear_geometry(stride)[0] != 0
    assert by_name["s32_ragged"].n == 1283


def test_the_generator_is_deterministic():
    a = FM.sweep_batch(320)
    FM._CACHE.pop(("sweep", 320, 1100))
    b = FM.sweep_batch(320)
    assert a.q is not b.q and np.array_equal(a.q, b.q) and np.array_equal(a.lens, b.lens)


def test_the_oracle_ignores_what_lies_past_a_read(oracle):
    """The batches leave random bytes past a read's length: the oracle, like the kernels, must not look at them."""
    b = FM.sweep_batch(320)
    zeroed = np.where(np.arange(b.stride)[None, :] < b.lens[:, None], b.q, 0).astype(np.uint8)
    got, want = oracle.filter_batch(b.q, lens=b.lens, alpha=b.alpha), oracle.filter_batch(zeroed, lens=b.lens, alpha=b.alpha)
    assert all(np.array_equal(g, w, equal_nan=True) for g, w in zip(got, want))


def test_listed_batches_plant_exactly_m_reads(oracle):
    for m, ragged in [(m, r) for m in FM.LISTED_M for r in (False, True)]:
        b, at, exp = FM.listed_batch(oracle, m, ragged)
        live = np.arange(b.stride)[None, :] < b.lens[:, None]
        back = (exp[3] > 2) | (live & (b.q == 255)).any(1)
        assert len(at) == m and at[0] == 0 and (m == 1 or at[-1] == b.n - 1) and np.array_equal(np.flatnonzero(back), at)
        model = FM.Model(b.q, b.lens, b.alpha)
        assert model.unsure_share <= FM.UNSURE_MAX and int((~model.sure[at]).sum()) <= FM.UNSURE_MAX * m, (b.name, model.unsure_share)


# ---- the decode rules ------------------------------------------------------------------------------------------------

def _pack_rows(lib, seq, qual, lens, offset):
    """mpb_pack_batch_ascii row by row -> (matrix, accepted mask): the packer refuses a row with an undecodable byte."""
    n, stride = seq.shape
    out = np.zeros((n, stride), np.uint8)
    ok = np.zeros(n, bool)
    got_len = np.zeros(1, np.int32)
    for i in range(n):
        L = int(lens[i])
        off = np.array([0, L], np.int64)
        s, ql = seq[i, :L].tobytes() + b"\0", qual[i, :L].tobytes() + b"\0"
        rc = lib.mpb_pack_batch_ascii(s, ql, off.ctypes.data, 1, offset, 0, stride, out[i].ctypes.data, got_len.ctypes.data)
        ok[i] = rc == 0 and got_len[0] == L
    return out, ok


@pytest.mark.parametrize("offset", FM.SWAR_OFFSETS + FM.BYTE_OFFSETS)
def test_decode_rule_is_the_host_packer(offset):
    from moira_amd import _lib as L
    lib = L.load()
    seq, qual, lens = FM.decode_inputs()
    assert seq.shape == (FM.DECODE_N, FM.DECODE_STRIDE) and set(lens % 16) == set(range(16)) and lens.min() == 0
    assert len(np.unique(seq.astype(np.int64) * 256 + qual)) == 65536                     # every letter meets every quality
    assert all((seq == v).any() for v in FM.N_NEIGHBOURS)
    # as it is, nearly every row holds a byte the packer refuses: the rows it accepts, then the same letters with every quality
    # folded into the offset's decodable range
    lo, hi = max(offset, 0), min(255, offset + 254)
    folded = (lo + qual.astype(np.int64) % (hi - lo + 1)).astype(np.uint8) if hi >= lo else qual
    accepted = 0
    for ql in (qual, folded):
        want, bad = FM.decode_rule(seq, ql, lens, offset)
        got, ok = _pack_rows(lib, seq, ql, lens, offset)
        live = np.arange(seq.shape[1])[None, :] < lens[:, None]
        qv = ql.astype(np.int64) - offset
        clean = ~(live & ((qv < 0) | (qv > 254))).any(1)
        assert np.array_equal(ok, clean) and bad == int((live & ((qv < 0) | (qv > 254))).sum())
        assert np.array_equal(got[ok], want[ok])
        accepted += int(ok.sum())
    assert accepted >= (FM.DECODE_N if hi >= lo else 1)           # offsets 256 and 300: only the read of no bases
