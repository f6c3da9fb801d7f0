"""Inputs shared by the tests of the fused BGZF FASTQ call (mpb_filter_bgzf_fastq_host; Engine.filter_bgzf_fastq; the CLI's
three switches together): tests/test_bgzf_fastq_args.py and tests/test_gpu_bgzf_fastq.py.  Members come from
tests/helpers/inflate_inputs.py's frame() and deflate(), texts from tests/helpers/fastq_index_texts.py and the golden reads."""
import gzip
import io
import os

import numpy as np

from helpers import inflate_inputs as I

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
GOLD = os.path.join(ROOT, "tests", "golden")


def golden_text(records=None):
    """The golden single-end reads as text; the first `records` of them when given."""
    text = gzip.open(os.path.join(GOLD, "test1.fastq.gz"), "rb").read()
    if records is None:
        return text
    lines = text.split(b"\n")
    return b"\n".join(lines[:4 * records]) + b"\n"


def member(text, level=6):
    return I.frame(I.deflate(text, level), text)


def cut(text, size, level=6):
    """`text` as members of `size` bytes each (the last one shorter)."""
    return [member(text[at:at + size], level) for at in range(0, len(text), size)]


def batch_of(members):
    """(data uint8, offs, sizes, out_offs) of members laid back to back."""
    blob, offs, sizes, out_offs = I.layout(members) if members else (b"", np.zeros(0, np.int64), np.zeros(0, np.int32), np.zeros(1, np.int64))
    return np.frombuffer(blob, np.uint8), offs, sizes, out_offs


def scan(blob):
    """The one batch GzipReader.read_members makes of a BGZF file's bytes."""
    from moira_amd import fastio as F
    r = F.GzipReader(io.BytesIO(blob), threads=2)
    try:
        b = r.read_members()
        assert b is not None and r.read_members() is None
        return b
    finally:
        r.close()


def inflated(batch):
    """The batch's text by zlib."""
    return gzip.decompress(batch[0].tobytes()) if len(batch[1]) else b""
