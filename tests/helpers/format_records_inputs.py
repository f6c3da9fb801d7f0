"""The cases of mpb_format_records_host beyond mpb_format_text_host's (tests/helpers/format_inputs.py): the ";ee=%.2f;size=1;"
suffix for kinds 0, 1, 2 and 4, and kind 4, the contigs.report line.  Shared by the host lane model
(tests/test_format_records_model.py) and the GPU tests (tests/test_gpu_format_records.py).  A case is format_inputs' dict; `kw`
may also hold `ee` (float64, one per selected record, by position) and `aux` (int32[n_records, 3], by record).  The reference of
every case is fastio.format_records(ee=) or, for kind 4, fastio.format_report on the same arguments."""
from fractions import Fraction

import numpy as np

from helpers import format_inputs as X
from moira_amd import fastio as F

REPORT = F.FMT_REPORT
KINDS = (F.FMT_FASTA, F.FMT_QUAL, F.FMT_FASTQ, REPORT)
KIND_NAME = dict(X.KIND_NAME)
KIND_NAME[REPORT] = "report"
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
AUX_VALUES = (0, 9, 10, 99, 100, -1, INT32_MIN, INT32_MAX)
N_RECORDS = len(AUX_VALUES) ** 3                           # every value in each column, against every value in the others


def ee_values():
    """The issue's list: signed zeros, exact ties of the hundredths, values whose decimal form looks like a tie but whose binary
    value is not one, the ends of the domain, integers, and both neighbours of 100 values k/200 + 0.0025."""
    v = [0.0, -0.0, 0.125, 0.375, 0.625, 2.5, 0.005, 0.015, 0.995, 9.995, 99.995, 65535.995, 1e-300, 5e-324, -0.001, float(2 ** 53 - 1),
         -float(2 ** 53 - 1), 1.0, 7.0, 100.0, 12345678.0, -3.0, -0.125, -0.375, 0.994999999, 1234.5678]
    for k in range(100):
        x = k / 200.0 + 0.0025
        v += [float(np.nextafter(x, -np.inf)), x, float(np.nextafter(x, np.inf))]
    return np.array(v, np.float64)


EE = ee_values()
OUTSIDE = (float("nan"), float("inf"), -float("inf"), float(2 ** 53), -float(2 ** 53))


def rounds_down_on_a_tie(v):
    """True where 100 |v| lies exactly half way between two integers and "%.2f" takes the lower (even) one."""
    t = Fraction(abs(float(v))) * 100
    return t.denominator == 2 and (t.numerator // 2) % 2 == 0


def base_text():
    """N_RECORDS records whose header tokens have 1, 15, 16, 17 and 300 bytes, with and without ':'."""
    rng = np.random.default_rng(21)
    recs = []
    for i in range(N_RECORDS):
        tl = X.TOKEN_LENGTHS[i % len(X.TOKEN_LENGTHS)]
        n = 1 + (i * 7) % 40
        recs.append((X.token(i, tl, colons=(i // 5) % 2 == 1), X.bases(rng, n), X.quals(rng, n)))
    return X.build(recs)


def base_aux():
    a = np.array(AUX_VALUES, np.int64)
    i = np.arange(N_RECORDS)
    return np.stack([a[i % 8], a[(i // 8) % 8], a[(i // 64) % 8]], 1).astype(np.int32)


def ee_for(n, shift=0):
    return EE[(np.arange(n) + shift) % len(EE)]


def want(c):
    """fastio.format_records / fastio.format_report on the case's arguments."""
    kw = dict(c["kw"])
    sel = np.arange(len(c["idx"]), dtype=np.int64) if c["sel"] is None else c["sel"]
    if kw["kind"] != REPORT:
        kw.pop("aux", None)
        return bytes(F.format_records(c["text"], c["idx"], sel, **kw))
    return bytes(F.format_report(c["text"], c["idx"], sel, kw["aux"], relabel=kw.get("relabel"), relabel_index=kw.get("relabel_index"),
                                 ee=kw.get("ee")))


def main_cases():
    """Kinds 0, 1, 2 and 4, each with and without ee, relabel on and off, labels on and off (a report line takes none)."""
    text, idx = base_text()
    n = len(idx)
    aux = base_aux()
    ri = np.array([X.RELABEL_INDEXES[i % len(X.RELABEL_INDEXES)] for i in range(n)], np.int64)
    lab = np.array([(i % 17) - 1 for i in range(n)], np.int32)
    out = []
    for k in KINDS:
        for with_ee in (False, True):
            for with_relabel in (False, True):
                for with_labels in ((False,) if k == REPORT else (False, True)):
                    kw = dict(kind=k)
                    if with_ee:
                        kw["ee"] = ee_for(n)
                    if with_relabel:
                        kw.update(relabel="Seq_", relabel_index=ri)
                    if with_labels:
                        kw.update(labels=X.LABELS, label_id=lab)
                    if k == REPORT:
                        kw["aux"] = aux
                    out.append(X.case("%s_e%d_r%d_l%d" % (KIND_NAME[k], with_ee, with_relabel, with_labels), text, idx, **kw))
    return out


def sel_cases():
    """Reverse order and repeats: aux goes by record, ee by position."""
    text, idx = base_text()
    n = len(idx)
    aux = base_aux()
    rng = np.random.default_rng(22)
    sels = dict(reversed=np.arange(n)[::-1].copy(), repeats=rng.integers(0, n, 700), one=np.array([n - 1]), empty=np.zeros(0, np.int64))
    out = []
    for name, s in sels.items():
        out.append(X.case("sel_%s_report" % name, text, idx, sel=s, kind=REPORT, aux=aux, ee=ee_for(len(s), 3)))
        out.append(X.case("sel_%s_report_plain" % name, text, idx, sel=s, kind=REPORT, aux=aux))
        out.append(X.case("sel_%s_fastq" % name, text, idx, sel=s, kind=F.FMT_FASTQ, ee=ee_for(len(s), 5)))
    return out


def report_ignores_sequence_columns():
    """A report line reads the header alone: rows whose sequence and quality columns hold anything are taken."""
    text, idx = X.count_text(20, 14)
    a = idx.copy()
    a[:, 2] = -9
    a[:, 3] = 1 << 45
    a[:, 4] = -7
    a[:, 5] = 1 << 50
    return X.case("report_any_seq_columns", text, a, kind=REPORT, aux=np.arange(60, dtype=np.int32).reshape(20, 3) - 30, ee=ee_for(20))


def count_cases():
    """0, 1, 32, 33 and 1025 selected records: none, one workgroup, one more, one more than a trip of k_fmt_scan."""
    out = []
    for n in (0, 1, 32, 33, 1025):
        text, idx = X.count_text(n, 23)
        aux = (np.arange(3 * n, dtype=np.int64) * 7919 % 2003 - 1000).astype(np.int32).reshape(n, 3)
        out.append(X.case("count_%d_report" % n, text, idx, kind=REPORT, aux=aux, ee=ee_for(n, 1)))
        out.append(X.case("count_%d_fasta" % n, text, idx, kind=F.FMT_FASTA, ee=ee_for(n, 2)))
    return out


def all_cases():
    return main_cases() + sel_cases() + count_cases() + [report_ignores_sequence_columns()]


def tie_cases():
    """For the half-up sensitivity build: cases whose ee hold a tie that rounds down, and cases that hold none."""
    text, idx = X.count_text(12, 24)
    aux = np.zeros((12, 3), np.int32)
    ties = np.array([0.125, 0.625, 2.125, -0.125] * 3)
    plain = np.array([0.375, 0.875, 0.005, 0.015, 0.995, 2.5, 1.0, 0.13, -0.375, 9.995, 0.0, 65535.995])
    out = []
    for k in KINDS:
        kw = dict(aux=aux) if k == REPORT else {}
        out.append(X.case("ties_%s" % KIND_NAME[k], text, idx, kind=k, ee=ties, **kw))
        out.append(X.case("noties_%s" % KIND_NAME[k], text, idx, kind=k, ee=plain, **kw))
    return out


def sign_cases():
    """For the dropped-minus sensitivity build: report cases with and without a negative aux value, and another kind."""
    text, idx = X.count_text(12, 25)
    neg = np.arange(36, dtype=np.int32).reshape(12, 3)
    neg[5, 1] = -4
    neg[7, 2] = INT32_MIN
    pos = np.arange(36, dtype=np.int32).reshape(12, 3)
    pos[3, 0] = INT32_MAX
    return [X.case("aux_negative", text, idx, kind=REPORT, aux=neg), X.case("aux_negative_ee", text, idx, kind=REPORT, aux=neg, ee=ee_for(12)),
            X.case("aux_positive", text, idx, kind=REPORT, aux=pos), X.case("aux_none_fastq", text, idx, kind=F.FMT_FASTQ, ee=ee_for(12))]


def refused_cases():
    """(case, the first bad k): an ee outside the domain, a sel outside the records (so aux is never read out of range), damaged
    header columns and a negative relabel_index of a report line."""
    text, idx = X.count_text(50, 26)
    n, T = len(idx), len(text)
    aux = np.arange(3 * n, dtype=np.int32).reshape(n, 3)
    out = []
    for j, v in enumerate(OUTSIDE):
        for k in (F.FMT_FASTA, F.FMT_QUAL, F.FMT_FASTQ, REPORT):
            ee = ee_for(n)
            ee = ee.copy()
            ee[9 + j] = v
            kw = dict(aux=aux) if k == REPORT else {}
            out.append((X.case("ee_outside_%d_%s" % (j, KIND_NAME[k]), text, idx, kind=k, ee=ee, **kw), 9 + j))
    for name, v in (("sel_n", n), ("sel_neg", -1), ("sel_huge", 1 << 62), ("sel_min", -(1 << 63))):
        s = np.arange(n)
        s[11] = v
        out.append((X.case("report_%s" % name, text, idx, sel=s, kind=REPORT, aux=aux), 11))

    def damaged(name, row, col, value):
        a = idx.copy()
        a[row, col] = value
        out.append((X.case(name, text, a, kind=REPORT, aux=aux, ee=ee_for(n)), row))
    damaged("report_hdr_off_past", 20, 0, T + 5)
    damaged("report_hdr_one_past", 49, 0, T - int(idx[49, 1]) + 1)
    damaged("report_hdr_off_neg", 20, 0, -1)
    damaged("report_hdr_len_neg", 20, 1, -1)
    damaged("report_hdr_len_huge", 20, 1, 1 << 40)
    ri = np.arange(n)
    ri[33] = -1
    out.append((X.case("report_relabel_index_neg", text, idx, kind=REPORT, aux=aux, relabel="S", relabel_index=ri), 33))
    both = ee_for(n).copy()
    both[40] = float("nan")
    s = np.arange(n)
    s[30] = n
    out.append((X.case("report_first_of_two", text, idx, sel=s, kind=REPORT, aux=aux, ee=both), 30))
    return out
