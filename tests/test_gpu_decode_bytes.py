"""decode4 / decode4_bytes / decode16 on the GPU, byte by byte: the word-wide arithmetic (borrow-free per-byte subtract, the
fallback for a character below the offset, Q0 -> 1, 'N' / 'n' found by | 0x20) against the plain numpy statement of the rules
(tests/helpers/front_end_model.py: decode_rule) on a matrix in which every quality byte meets every letter byte -- qualities
>= 0x80, letters one bit away from 'N' / 'n' -- at offsets 1 .. 255 (word-wide path) and 0, negative, > 255 (byte path), through
both entries that decode: mpb_decode_ascii_device and mpb_decode_classify_device + mpb_filter_device_classified."""
import numpy as np
import pytest

from helpers import front_end_model as FM
from helpers.device_runs import same

pytestmark = pytest.mark.gpu

OFFSETS = FM.SWAR_OFFSETS + FM.BYTE_OFFSETS


@pytest.fixture(scope="module")
def eng():
    from moira_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def text(eng):
    """The letters and quality characters resident in HBM, with the buffers every case writes to."""
    seq, qual, lens = FM.decode_inputs()
    n, stride = seq.shape
    d = dict(seq=eng.alloc(n * stride).upload(seq), qual=eng.alloc(n * stride).upload(qual), len=eng.alloc(n * 4).upload(lens),
             out=eng.alloc(n * stride), err=eng.alloc(4), ee=eng.alloc(n * 8), ns=eng.alloc(n * 4), ps=eng.alloc(n))
    yield d
    for b in d.values():
        b.free()


def _layout(ragged):
    seq, qual, lens = FM.decode_inputs()
    return seq, qual, (lens if ragged else np.full(len(lens), FM.DECODE_STRIDE, np.int32))


def test_the_inputs_meet_what_they_are_for():
    seq, qual, lens = FM.decode_inputs()
    assert len(np.unique(seq.astype(np.int64) * 256 + qual)) == 65536 and all((seq == v).any() for v in FM.N_NEIGHBOURS)
    assert set(lens % 16) == set(range(16)) and lens.min() == 0 and lens.max() == FM.DECODE_STRIDE
    for offset in OFFSETS:                          # every branch of the rule is taken: below the offset, Q0, above 254
        qv = qual.astype(np.int64) - offset
        assert ((qv < 0).any() or offset <= 0) and ((qv == 0).any() or not 0 <= offset <= 255) and ((qv > 254).any() or offset > 0)


@pytest.mark.parametrize("ragged", [False, True], ids=["fixed272", "ragged"])
@pytest.mark.parametrize("offset", OFFSETS)
def test_decode_ascii_device(eng, text, offset, ragged):
    seq, qual, lens = _layout(ragged)
    n, stride = seq.shape
    want, bad = FM.decode_rule(seq, qual, lens, offset)
    text["out"].upload(np.full(n * stride, 0xAB, np.uint8))                     # every byte of a row must be written
    text["err"].upload(np.zeros(1, np.int32))
    eng.decode_ascii_device(text["seq"], text["qual"], n, stride, text["out"], d_len=text["len"] if ragged else None,
                            fixed_len=0 if ragged else stride, fastq_offset=offset, d_err=text["err"])
    got = text["out"].download(np.uint8, n * stride).reshape(n, stride)
    diff = np.argwhere(got != want)
    assert len(diff) == 0, (offset, len(diff), [(int(i), int(t), hex(seq[i, t]), hex(qual[i, t]), int(got[i, t]), int(want[i, t]))
                                                for i, t in diff[:6]])
    assert text["err"].download(np.int32, 1)[0] == bad, offset


@pytest.mark.parametrize("ragged", [False, True], ids=["fixed272", "ragged"])
@pytest.mark.parametrize("offset", OFFSETS)
def test_decode_classify_then_filter(eng, oracle, text, offset, ragged):
    seq, qual, lens = _layout(ragged)
    n, stride = seq.shape
    want, bad = FM.decode_rule(seq, qual, lens, offset)
    text["out"].upload(np.full(n * stride, 0xAB, np.uint8))
    text["err"].upload(np.zeros(1, np.int32))
    c = eng.filter_ascii_device(text["seq"], text["qual"], n, stride, text["out"], d_len=text["len"] if ragged else None,
                                fixed_len=0 if ragged else stride, fastq_offset=offset, d_ee=text["ee"], d_ns=text["ns"],
                                d_pass=text["ps"], d_err=text["err"])
    got = text["out"].download(np.uint8, n * stride).reshape(n, stride)
    diff = np.argwhere(got != want)
    assert len(diff) == 0, (offset, len(diff), [(int(i), int(t), hex(seq[i, t]), hex(qual[i, t]), int(got[i, t]), int(want[i, t]))
                                                for i, t in diff[:6]])
    assert text["err"].download(np.int32, 1)[0] == bad, offset
    ee, ns, ps, _ = oracle.filter_batch(want, lens=lens, threads=8)
    assert same(text["ee"].download(np.float64, n), ee) and np.array_equal(text["ns"].download(np.int32, n), ns)
    assert np.array_equal(text["ps"].download(np.uint8, n), ps) and (c.n_reads, c.n_pass) == (n, int(ps.sum()))
