"""Shared by the directed GPU test files: one batch through one entry of the library, results back as numpy arrays."""
import ctypes as C

import numpy as np

SENT_EE, SENT_NS, SENT_PS = -7.0, -7, 9          # what result arrays hold before a call: never a result


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


class Resident:
    """A host batch uploaded once: q (and lens for a ragged batch) in HBM, result arrays with guard elements on each side (two in
    front, so that the arrays themselves stay aligned to 16, 8 and 2 bytes when res_offset is 0).
    q_offset: bytes the matrix lies behind its (256-byte aligned) allocation; res_offset: elements the result arrays do."""

    def __init__(self, eng, q, lens=None, q_offset=0, res_offset=0):
        self.eng, self.n, self.stride = eng, q.shape[0], q.shape[1]
        n = self.n
        self.q_offset, self.k = int(q_offset), int(res_offset)
        self.d_q = eng.alloc(max(1, q.nbytes) + self.q_offset + 256)
        raw = np.zeros(q.nbytes + self.q_offset, np.uint8)
        raw[self.q_offset:] = np.ascontiguousarray(q).reshape(-1)
        self.d_q.upload(raw)
        self.d_len = eng.alloc(max(1, n) * 4).upload(np.ascontiguousarray(lens, np.int32)) if lens is not None else None
        m = n + 3 + self.k                        # [2 guards][k elements of offset][n results][guard]
        self.d_ee, self.d_ns, self.d_pass = eng.alloc(m * 8), eng.alloc(m * 4), eng.alloc(m)
        self.bufs = [b for b in (self.d_q, self.d_len, self.d_ee, self.d_ns, self.d_pass) if b is not None]

    def reset(self):
        m = self.n + 3 + self.k
        self.d_ee.upload(np.full(m, SENT_EE))
        self.d_ns.upload(np.full(m, SENT_NS, np.int32))
        self.d_pass.upload(np.full(m, SENT_PS, np.uint8))

    def ptrs(self):
        o = 2 + self.k
        return self.d_q.ptr + self.q_offset, self.d_ee.ptr + 8 * o, self.d_ns.ptr + 4 * o, self.d_pass.ptr + o

    def results(self):
        """(ee, ns, pass) and whether every element outside the n results still holds its sentinel."""
        m, o, n = self.n + 3 + self.k, 2 + self.k, self.n
        ee, ns, ps = self.d_ee.download(np.float64, m), self.d_ns.download(np.int32, m), self.d_pass.download(np.uint8, m)
        out = np.ones(m, bool)
        out[o:o + n] = False
        intact = (ee[out] == SENT_EE).all() and (ns[out] == SENT_NS).all() and (ps[out] == SENT_PS).all()
        return ee[o:o + n], ns[o:o + n], ps[o:o + n], bool(intact)

    def run(self, fixed_len=None, want_counts=True, **kw):
        """mpb_filter_device -> (ee, ns, pass, counts, path, guards intact)."""
        eng = self.eng
        self.reset()
        q, ee, ns, ps = self.ptrs()
        c = eng.filter_device(q, self.n, self.stride, d_len=self.d_len if fixed_len is None else None,
                              fixed_len=0 if fixed_len is None else int(fixed_len), d_ee=ee, d_ns=ns, d_pass=ps,
                              params=eng.params(**kw), want_counts=want_counts)
        if not want_counts:
            eng.synchronize()
        ee_, ns_, ps_, intact = self.results()
        return ee_, ns_, ps_, c, eng.last_path(), intact

    def free(self):
        for b in self.bufs:
            b.free()


def classified_pair(eng, q, lens, fixed_len=None, front_end=False, **kw):
    """The batch as FASTQ text in HBM (mpb_encode_ascii_device) through mpb_decode_classify_device +
    mpb_filter_device_classified -> (ee, ns, pass, counts); with front_end=True the result arrays lie between guard elements
    (two in front, one behind, as Resident's) and the tuple goes on with the budgets and the class histogram the library reports
    after the pair, the packed matrix the decode pass wrote, and whether every guard still holds its sentinel."""
    n, stride = q.shape
    g = 2 if front_end else 0                         # guard elements in front of the results (one behind)
    m = n + (3 if front_end else 0)
    d_q, d_seq, d_qual, d_out = (eng.alloc(max(1, n * stride)) for _ in range(4))
    d_len = eng.alloc(max(1, n) * 4).upload(np.ascontiguousarray(lens, np.int32)) if fixed_len is None else None
    d_ee, d_ns, d_pass = eng.alloc(m * 8), eng.alloc(m * 4), eng.alloc(m)
    try:
        d_q.upload(np.ascontiguousarray(q))
        eng.encode_ascii_device(d_q, n, stride, d_seq, d_qual)
        d_ee.upload(np.full(m, SENT_EE))
        if front_end:
            d_ns.upload(np.full(m, SENT_NS, np.int32))
            d_pass.upload(np.full(m, SENT_PS, np.uint8))
        c = eng.filter_ascii_device(d_seq, d_qual, n, stride, d_out, d_len=d_len, fixed_len=0 if fixed_len is None else fixed_len,
                                    d_ee=d_ee.ptr + 8 * g, d_ns=d_ns.ptr + 4 * g, d_pass=d_pass.ptr + g, params=eng.params(**kw))
        ee, ns, ps = d_ee.download(np.float64, m), d_ns.download(np.int32, m), d_pass.download(np.uint8, m)
        out = ee[g:g + n], ns[g:g + n], ps[g:g + n], c
        if front_end:
            outside = np.ones(m, bool)
            outside[g:g + n] = False
            intact = (ee[outside] == SENT_EE).all() and (ns[outside] == SENT_NS).all() and (ps[outside] == SENT_PS).all()
            out += (eng.read_budgets(n), eng.class_histogram(), d_out.download(np.uint8, n * stride).reshape(n, stride), bool(intact))
        return out
    finally:
        for b in (d_q, d_seq, d_qual, d_out, d_len, d_ee, d_ns, d_pass):
            if b is not None:
                b.free()


def seq_and_quals(row, n):
    """A packed row as the per-read entry wants it: 'N' / 'n' where the byte says so (their scores do not matter)."""
    row = np.asarray(row[:n])
    seq = "".join("N" if v == 0 else "n" if v == 255 else "A" for v in row)
    return seq, [20 if v in (0, 255) else int(v) for v in row]


def matrix_offset_is_refused(eng, res, offset):
    """rc of mpb_filter_device for the resident matrix moved `offset` bytes (results untouched)."""
    prm = eng.params(no_narrow=True)
    q, ee, ns, ps = res.ptrs()
    return eng.lib.mpb_filter_device(eng.ctx, C.c_void_p(q + offset), res.n, res.stride, None, 16, C.byref(prm),
                                     C.c_void_p(ee), C.c_void_p(ns), C.c_void_p(ps), None)
