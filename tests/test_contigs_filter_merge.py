"""The host side of the fused contig-and-filter call, without a device (a fake engine stands in for Engine.contigs_filter_text and
Engine.filter_text): moira_amd.contig.contigs_from_fastq_filtered must rebuild the pairs the device handed back with the host
aligner, ask filter_text for exactly the pairs the fused call did not filter, and return what the all-host path returns; the
CLI's helpers must take the fused call only with both switches, and send a chunk whose filter was refused down the
--device_pack branch.  The call itself on the GPU: tests/test_gpu_contigs_filter.py."""
import types

import numpy as np
import pytest

from helpers import contig_pairs as P
from moira_amd import _lib as L
from moira_amd import cli
from moira_amd import contig as CT
from moira_amd import engine as E


def make_pairs(n=60, seed=9):
    rng = np.random.default_rng(seed)
    return [P.make_pair(rng, int(rng.integers(5, 200)), int(rng.integers(5, 200)), ("overlap", "unrelated", "contained")[k % 3]) for k in range(n)]


def fake_results(idx, sel, max_len):
    """What the fake filter says of the records sel: ee = packed length + 0.5, has_n at the even positions."""
    ln = idx[sel, 5] if not max_len else np.minimum(idx[sel, 5], max_len)
    return ln + 0.5, sel % 2 == 0


class FakeEngine:
    """contigs_filter_text: the host's contigs, with `not_done` handed back (slot 0xFF, index and aux rows garbage) and
    `not_filtered` built but left unfiltered; filter_text: fake_results, and a record of what it was asked for."""

    def __init__(self, texts, not_done=(), not_filtered=(), error=None):
        self.host = CT.contigs_from_fastq(*texts, 33, threads=2)
        self.not_done, self.not_filtered, self.error = np.array(not_done, int), np.array(not_filtered, int), error
        self.asked, self.fused_calls, self.plain_calls = [], 0, 0

    def contigs_text(self, fbuf, fidx, rbuf, ridx, *a, rec_cap=None, **kw):
        self.plain_calls += 1
        n = len(fidx)
        cbuf, cidx, aux = (x.copy() for x in self.host)
        assert rec_cap == len(cbuf) // n
        return E.ContigResult(cbuf, cidx, aux, np.ones(n, bool), rec_cap, n, 0, None, None, None)

    def contigs_filter_text(self, fbuf, fidx, rbuf, ridx, *a, rec_cap=None, max_len=0, **kw):
        self.fused_calls += 1
        n = len(fidx)
        cbuf, cidx, aux = (x.copy() for x in self.host)
        assert rec_cap == len(cbuf) // n
        done = np.ones(n, bool)
        done[self.not_done] = False
        cbuf.reshape(n, rec_cap)[~done] = 0xFF
        cidx[~done] = -(2 ** 40)
        aux[~done] = -7
        filtered = done.copy()
        filtered[self.not_filtered] = False
        if self.error is not None:
            filtered[:] = False
        ee, has_n = fake_results(self.host[1], np.arange(n), max_len)
        ee, has_n = np.where(filtered, ee, np.nan), has_n & filtered
        base = E.ContigResult(cbuf, cidx, aux, done, rec_cap, int(done.sum()), int((~done).sum()), None, None, None)
        return E.ContigFilterResult(base, ee, np.zeros(n, np.int32), filtered.copy(), np.zeros(n, np.int32), has_n, filtered,
                                    int(filtered.sum()), 0, self.error)

    def filter_text(self, buf, idx, sel=None, max_len=0, **kw):
        sel = np.arange(len(idx)) if sel is None else np.asarray(sel)
        self.asked.append(sel.tolist())
        ee, has_n = fake_results(np.asarray(idx), sel, max_len)
        return E.TextFilterResult(ee, np.zeros(len(sel), np.int32), np.ones(len(sel), bool), np.zeros(len(sel), np.int32), has_n, len(sel), 0)


@pytest.mark.parametrize("max_len", [0, 100])
@pytest.mark.parametrize("not_done, not_filtered", [((), ()), ((3, 4, 17, 59), ()), ((0, 30), (1, 2, 31, 58)), (tuple(range(60)), ())],
                         ids=["all_filtered", "handed_back", "handed_back_and_unfiltered", "none_built"])
def test_merged_result_equals_the_all_host_result(not_done, not_filtered, max_len):
    texts = P.texts(make_pairs())
    eng = FakeEngine(texts, not_done, not_filtered)
    cbuf, cidx, aux, ee, has_n, err = CT.contigs_from_fastq_filtered(*texts, 33, threads=2, engine=eng, max_len=max_len)
    hbuf, hidx, haux = eng.host
    assert err is None and eng.fused_calls == 1
    assert np.array_equal(cidx, hidx) and np.array_equal(aux, haux) and P.records(cbuf, cidx) == P.records(hbuf, hidx)
    want_ee, want_n = fake_results(hidx, np.arange(len(hidx)), max_len)
    assert np.array_equal(ee, want_ee) and np.array_equal(has_n, want_n)
    rest = sorted(set(not_done) | set(not_filtered))
    assert eng.asked == ([rest] if rest else [])             # exactly the unfiltered positions, in order, in one call


def test_the_rest_goes_through_the_callers_own_text_filter():
    texts = P.texts(make_pairs())
    eng = FakeEngine(texts, (5,), (6,))
    seen = []

    def backend_text(buf, idx, sel):
        seen.append(sel.tolist())
        return np.full(len(sel), 2.5), np.ones(len(sel), bool)
    *_, ee, has_n, err = CT.contigs_from_fastq_filtered(*texts, 33, threads=2, engine=eng, backend_text=backend_text)
    assert seen == [[5, 6]] and eng.asked == [] and err is None
    assert ee[[5, 6]].tolist() == [2.5, 2.5] and has_n[[5, 6]].all()


def test_a_refused_filter_is_returned_not_raised_and_nothing_more_is_asked_of_the_device():
    texts = P.texts(make_pairs())
    boom = ValueError("quality exceeds the encodable maximum 254")
    boom.bad_record = 7
    eng = FakeEngine(texts, (3,), (), error=boom)
    cbuf, cidx, aux, ee, has_n, err = CT.contigs_from_fastq_filtered(*texts, 33, threads=2, engine=eng)
    assert err is boom and err.bad_record == 7 and eng.asked == []
    assert np.array_equal(cidx, eng.host[1]) and np.array_equal(aux, eng.host[2])        # the contigs are complete all the same
    with pytest.raises(ValueError, match="needs an engine"):
        CT.contigs_from_fastq_filtered(*texts, 33)


def test_a_refusal_of_the_rest_is_the_chunks_error_too():
    texts = P.texts(make_pairs())
    eng = FakeEngine(texts, (5,), ())
    boom = ValueError("Qualities must have positive values.")

    def backend_text(buf, idx, sel):
        raise boom
    cbuf, cidx, aux, ee, has_n, err = CT.contigs_from_fastq_filtered(*texts, 33, threads=2, engine=eng, backend_text=backend_text)
    assert err is boom and np.array_equal(cidx, eng.host[1]) and np.array_equal(aux, eng.host[2])


def run_args():
    return types.SimpleNamespace(alpha=0.005, ambigs="treat_as_errors", round=False, match=1, mismatch=-1, gap=-2, insert=20, deltaq=6,
                                 consensus_qscore="best", qscore_cap=40, trim_overlap=False, processors=2)


def fake_backend(eng):
    be = types.SimpleNamespace(engine=eng, text_calls=[])
    be.text_choice = lambda alpha, ambigs, round_, method="poisson_binomial", fast_discard=None: dict(alpha=alpha, ambigs=ambigs, round_=round_, uncert=1.0)

    def text(buf, idx, alpha, ambigs, round_, fastq_offset, max_len, lower_n_is_base, method="poisson_binomial", fast_discard=None, sel=None):
        be.text_calls.append(None if sel is None else sel.tolist())
        r = eng.filter_text(buf, idx, sel=sel, max_len=max_len)
        return r.ee, r.has_n
    be.text = text
    return be


def test_cli_helper_hands_the_results_on_with_the_chunk():
    texts = P.texts(make_pairs())
    eng = FakeEngine(texts, (2,), (9,))
    be = fake_backend(eng)
    chunk = cli._DeferredContigs(cli._Contigs(run_args()), *texts, 33, eng, fused=cli._TextFilter(be, run_args(), 33, 0, False, "poisson_binomial", None))
    buf, idx, aux, filtered = cli._filtered_where_built(chunk.build())
    assert eng.fused_calls == 1 and eng.plain_calls == 0 and be.text_calls == [[2, 9]]
    want_ee, want_n = fake_results(eng.host[1], np.arange(60), 0)
    assert np.array_equal(filtered[0], want_ee) and np.array_equal(filtered[1], want_n) and np.array_equal(idx, eng.host[1])


def test_cli_helper_sends_a_refused_chunk_down_the_device_pack_branch():
    """filter_error set: the chunk brings its contigs and no results, as a chunk of --device_contigs alone does, so the run's
    --device_pack branch filters it (and raises, or falls back and reports, as it always did); the helper asked for nothing."""
    texts = P.texts(make_pairs())
    eng = FakeEngine(texts, (2,), (), error=ValueError("Qualities must have positive values."))
    be = fake_backend(eng)
    chunk = cli._DeferredContigs(cli._Contigs(run_args()), *texts, 33, eng, fused=cli._TextFilter(be, run_args(), 33, 0, False, "poisson_binomial", None))
    buf, idx, aux, filtered = cli._filtered_where_built(chunk.build())
    assert filtered is None and be.text_calls == [] and np.array_equal(idx, eng.host[1])
    assert cli._filtered_where_built((buf, idx, aux)) == (buf, idx, aux, None)


def test_either_switch_alone_does_not_reach_the_fused_call():
    texts = P.texts(make_pairs())
    eng = FakeEngine(texts)
    be = fake_backend(eng)
    assert cli._fused_applies(True, True, False, be)
    assert not cli._fused_applies(True, False, False, be) and not cli._fused_applies(False, True, False, be)
    assert not cli._fused_applies(True, True, True, be)                               # --only_contig never reaches the device pack
    assert not cli._fused_applies(True, True, False, types.SimpleNamespace(engine=object(), text_choice=be.text_choice))
    # --device_contigs alone: the chunk is built through contigs_text, as before
    built = cli._DeferredContigs(cli._Contigs(run_args()), *texts, 33, eng).build()
    assert len(built) == 3 and eng.plain_calls == 1 and eng.fused_calls == 0 and be.text_calls == []


def test_the_library_and_the_engine_have_the_entry():
    lib = L.load()
    assert hasattr(lib, "mpb_contigs_filter_text_host") and "mpb_contigs_filter_text_host" in L.PROTOTYPES
    assert len(L.PROTOTYPES["mpb_contigs_filter_text_host"][1]) == len(L.PROTOTYPES["mpb_contigs_text_host"][1]) + 13
    assert callable(E.Engine.contigs_filter_text) and callable(CT.contigs_from_fastq_filtered)
    assert set(E.ContigFilterResult.__slots__) == {"ee", "ns", "passed", "lens", "has_n", "filtered", "n_pass", "n_overflow", "filter_error"}
    assert L.CONTIG_KERNEL_NAMES == {12: "contig", 13: "contig_rows"} and len(L.KERNEL_NAMES) == 12
