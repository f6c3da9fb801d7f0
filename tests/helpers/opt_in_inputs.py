"""The input families of tests/test_gpu_opt_in_models.py, shared with tests/test_opt_in_models.py (which checks on the CPU that
every one of them lies within the 1e-9 contract for both opt-in modes, so that a GPU failure can only be the kernel's)."""
import numpy as np

MODES = ("fma", "odds")
AMBIGS = ("treat_as_errors", "ignore", "disallow")


def mode_kw(mode):
    return {"fast_fma": True} if mode == "fma" else {"odds": True}


def synth300(oracle, n=20000, seed=4):
    """n x 300 bases at stride 320 -> (q, lens, fixed_len)."""
    q, lens = oracle.synth_fill(n, 320, fixed_len=300, seed=seed)
    return q, lens, 300


def ragged(oracle, n=40000):
    """n reads of 50..600 bases at stride 608."""
    q, lens = oracle.synth_fill(n, 608, min_len=50, max_len=600, seed=5)
    return q, lens, None


def wide_class_reads():
    """The reads of tests/test_gpu_parity.py::test_wide_classes: rows up to about 1000 (G = 2..64 classes)."""
    rng = np.random.default_rng(5)
    rows_q, lens = [], []
    for L, lo, hi in ((600, 1, 4), (1000, 1, 3), (1023, 1, 2), (500, 2, 8), (350, 1, 12), (800, 3, 20),
                      (1023, 1, 40), (97, 1, 3), (64, 1, 2), (33, 1, 2), (1023, 30, 41)):
        for _ in range(6):
            rows_q.append(rng.integers(lo, hi, L).astype(np.uint8))
            lens.append(L)
    q = np.zeros((len(lens), 1024), np.uint8)
    for i, r in enumerate(rows_q):
        q[i, :len(r)] = r
    q[3, 17] = 0
    q[5, 100] = 255
    return q, np.array(lens, np.int32), None


def tiny_fraction():
    """20000 reads of 16 bytes, length 12, random codes 1..254: many cross in row 1 with a tiny ee."""
    rng = np.random.default_rng(5)
    q = rng.integers(1, 255, (20000, 16)).astype(np.uint8)
    return q, np.full(len(q), 12, np.int32), 12


TINY_ALPHAS = (1e-5, 1e-3)
SWEEP_ALPHAS = (1e-5, 1e-4, 0.3, 0.9)


def threshold_picks(model_ee, k=6):
    """maxerrors values equal to reads' own model ee (ambigs ignore): spread over 0.5 .. 60."""
    u = np.unique(model_ee[(model_ee > 0.5) & (model_ee < 60)])
    return [float(x) for x in u[::max(1, len(u) // k)][:k]]


def host_pipeline(oracle):
    """600k x 300 at stride 320 (192 MB): four chunks of the host pipeline."""
    return synth300(oracle, n=600000, seed=6)


def clean(oracle, n=1 << 19):
    """The clean run's profile (Q33..Q40): a batch the default mode sends to the narrow pass."""
    q, lens = oracle.synth_fill(n, 320, fixed_len=300, seed=5, profile=1)
    return q, lens, 300


def classified(oracle):
    q, lens = oracle.synth_fill(50000, 320, fixed_len=300, seed=2, first_read=1000)
    return q, lens, 300
