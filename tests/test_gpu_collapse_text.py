"""The data-parallel part of collapse on the GPU (include/moira_pb.h: mpb_collapse_text_host; Engine.collapse_text; k_col_hash,
k_col_group, k_col_rep).  The oracle of hash is fastio.py2_hashes (mio_py2_hash), the oracle of rep a Python dict of truncated
sequences to first index; the cases are tests/helpers/collapse_inputs.py's, the ones the host lane model runs
(tests/test_collapse_lane_model.py, which also pins the byte compare with forged equal hashes: no GPU test can; long probe
walks from one start slot run here too, with real hashes found by search: crowded_cases)."""
import numpy as np
import pytest

from helpers import collapse_inputs as X
from moira_amd import engine as E
from moira_amd import fastio as F

pytestmark = pytest.mark.gpu

CASES = X.all_cases()
WANT = {}


def want(c):
    """The oracle of a case, computed once."""
    if c["name"] not in WANT:
        WANT[c["name"]] = X.want(c)
    return WANT[c["name"]]


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def golden():
    return X.golden_text()


def same(got, c):
    h, rep = want(c)
    assert got[0].dtype == np.uint64 and got[1].dtype == np.int32
    assert np.array_equal(got[0], h), (c["name"], "hash", np.flatnonzero(got[0] != h)[:5])
    assert np.array_equal(got[1], rep), (c["name"], "rep", np.flatnonzero(got[1] != rep)[:5])


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_the_uploaded_form_is_the_oracles_hash_and_first_equal_record(eng, c):
    same(eng.collapse_text(c["text"], c["idx"], max_len=c["max_len"]), c)


def test_two_calls_on_the_same_input_return_equal_arrays(eng):
    for c in X.big_cases() + X.crowded_cases():
        a, b = eng.collapse_text(c["text"], c["idx"]), eng.collapse_text(c["text"], c["idx"])
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_the_resident_form_is_the_uploaded_form_on_the_parsers_rows(eng, golden):
    text, idx = golden
    res = eng.filter_fastq(text)
    assert np.array_equal(res.idx, idx) and res.resident == eng.resident_text() > 0
    for max_len in (0, 100):
        up = eng.collapse_text(text, idx, max_len=max_len)
        for got in (eng.collapse_text(idx=res.idx, resident=res.resident, max_len=max_len),
                    eng.collapse_text(resident=res.resident, n=len(idx), max_len=max_len)):
            assert np.array_equal(got[0], up[0]) and np.array_equal(got[1], up[1])
        same(up, X.case("golden_100" if max_len else "golden", text, idx, max_len=max_len))
    assert eng.resident_text() == res.resident           # neither form ends the generation


def test_a_generation_made_stale_by_a_second_filter_call_is_not_resident(eng, golden):
    text, idx = golden
    first = eng.filter_fastq(text)
    second = eng.filter_fastq(text)
    assert second.resident == first.resident + 1
    with pytest.raises(E.NotResident):
        eng.collapse_text(idx=first.idx, resident=first.resident)
    with pytest.raises(E.NotResident):
        eng.collapse_text(resident=12345, n=len(idx))
    with pytest.raises(ValueError, match="is not the resident index's"):
        eng.collapse_text(resident=second.resident, n=len(idx) - 1)
    same(eng.collapse_text(idx=second.idx, resident=second.resident), X.case("golden", text, idx))


def test_a_format_call_and_a_collapse_call_share_a_generation_in_either_order(eng, golden):
    text, idx = golden
    w = bytes(F.format_records(text, idx, np.arange(len(idx)), F.FMT_FASTA))
    c = X.case("golden", text, idx)
    for order in ("format first", "collapse first"):
        res = eng.filter_fastq(text)
        calls = [lambda: eng.format_text(idx=res.idx, kind=F.FMT_FASTA, resident=res.resident),
                 lambda: eng.collapse_text(idx=res.idx, resident=res.resident)]
        if order == "collapse first":
            calls.reverse()
        got = [call() for call in calls]
        if order == "collapse first":
            got.reverse()
        assert got[0] == w, order
        same(got[1], c)
        assert eng.resident_text() == res.resident


def test_a_bad_row_of_the_uploaded_form_reports_its_record(eng):
    for c, bad in X.bad_row_cases():
        with pytest.raises(ValueError, match="record %d fails a check" % bad) as e:
            eng.collapse_text(c["text"], c["idx"])
        assert e.value.bad_record == bad, c["name"]
    c = X.small_cases()[3]
    same(eng.collapse_text(c["text"], c["idx"]), c)         # the context works on behind a refusal


def test_the_grouped_host_entry_verifies_the_devices_arrays(eng, golden):
    text, idx = golden
    ee = np.random.default_rng(3).random(len(idx))
    flags = np.zeros(len(idx), np.uint8)
    for max_len in (0, 100):
        h, rep = eng.collapse_text(text, idx, max_len=max_len)
        a, b = F.Collapse(4), F.Collapse(4)
        a.add(text, idx, ee, flags, max_len)
        b.add(text, idx, ee, flags, max_len, hash=h, rep=rep, verify=True)
        assert len(a) == len(b) > 0
        for x, y in zip(a.export(), b.export()):
            assert np.array_equal(x, y)
        a.close(), b.close()
