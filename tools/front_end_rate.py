#!/usr/bin/env python3
"""Time of the classification pass (k_prepass / k_classify_linear, the `prepass` span) per batch shape, with and without
lower-case 'n' in the reads: a lane that meets an 'n' sums its bytes a second time (mpb_kernels.hip), which clean input never pays.

    python tools/front_end_rate.py [reads in thousands, default 1000]

Shapes: fixed 300 / 320 and ragged .. 1024 and fixed 2000 / 2048 (the LONG instances) through mpb_filter_device, the list a forced
two-row narrow pass hands back (LISTED), and text through the classified-at-source pair.  `n` = 0.3 % of the bytes are 255.
Compare two builds by running it once per library (MOIRA_PB_LIB)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from moira_amd.engine import Engine  # noqa: E402


def batch(rng, n, stride, lo, with_n):
    q = rng.integers(lo, 42, (n, stride), dtype=np.uint8)
    if with_n:
        q[rng.random((n, stride), np.float32) < 0.003] = 255
    return q


def span(eng, call, reps=5):
    call()
    eng.timing(True)
    eng.timing_reset()
    for _ in range(reps):
        call()
    ms, k = eng.kernel_times()["prepass"]
    eng.timing(False)
    return ms / max(1, k)


def main():
    n = 1000 * (int(sys.argv[1]) if len(sys.argv) > 1 else 1000)
    rng = np.random.default_rng(7)
    lib = os.path.basename(os.environ.get("MOIRA_PB_LIB", "libmoira_pb.so"))
    with Engine(0) as eng:
        for name, reads, stride, fixed, lo in (("fixed 300/320", n, 320, 300, 25), ("ragged ..1024", n // 2, 1024, None, 30),
                                               ("fixed 2000/2048", n // 4, 2048, 2000, 33)):
            for with_n in (False, True):
                q = batch(rng, reads, stride, lo, with_n)
                d_q = eng.alloc(q.nbytes).upload(q)
                d_len = eng.alloc(reads * 4).upload(rng.integers(100, stride + 1, reads).astype(np.int32)) if fixed is None else None
                d_ee, d_ns, d_pass = eng.alloc(reads * 8), eng.alloc(reads * 4), eng.alloc(reads)
                kw = dict(d_len=d_len, fixed_len=fixed or 0, d_ee=d_ee, d_ns=d_ns, d_pass=d_pass)
                out = [span(eng, lambda: eng.filter_device(d_q, reads, stride, params=eng.params(no_narrow=True), **kw))]
                if stride == 320:
                    out.append(span(eng, lambda: eng.filter_device(d_q, reads, stride, params=eng.params(narrow_rows=2), **kw)))
                    back = eng.last_path()["n_fallback"]
                    d_seq, d_qual, d_out = (eng.alloc(q.nbytes) for _ in range(3))
                    eng.encode_ascii_device(d_q, reads, stride, d_seq, d_qual)
                    out.append(span(eng, lambda: eng.filter_ascii_device(d_seq, d_qual, reads, stride, d_out, **kw)))
                    for b in (d_seq, d_qual, d_out):
                        b.free()
                    extra = "  listed (%d handed back) %.3f ms  text %.3f ms" % (back, out[1], out[2])
                else:
                    extra = ""
                print("%s  %-16s %8d reads  %-7s prepass %.3f ms%s" % (lib, name, reads, "with n" if with_n else "clean", out[0], extra),
                      flush=True)
                for b in (d_q, d_len, d_ee, d_ns, d_pass):
                    if b is not None:
                        b.free()


if __name__ == "__main__":
    main()
