"""mpb_bgzf_member_rows (host only, no context): the validated rows of k_bgzf_inflate against struct parsing of the members, every
header defect (out_len = -1 and a reason, never an error return), and the argument errors."""
import ctypes as C
import struct

import numpy as np
import pytest

from helpers import inflate_inputs as I
from moira_amd import _lib as L
from moira_amd import cli
from moira_amd import fastio as F


def rows_of(blob, offs, sizes, out_offs, n=None, why=True):
    lib = L.load()
    n = len(offs) if n is None else n
    rows = (L.BgzfMemberRow * max(n, 1))()
    crc, reason = np.zeros(max(n, 1), np.uint32), np.full(max(n, 1), 99, np.uint8)
    buf = np.frombuffer(bytes(blob), np.uint8) if len(blob) else np.zeros(1, np.uint8)
    rc = lib.mpb_bgzf_member_rows(buf.ctypes.data, len(blob), offs.ctypes.data, sizes.ctypes.data, out_offs.ctypes.data, n,
                                  C.addressof(rows), crc.ctypes.data, reason.ctypes.data if why else None)
    return rc, [(r.stream_off, r.out_off, r.stream_len, r.out_len) for r in rows[:n]], crc[:n], reason[:n]


def test_rows_and_crcs_equal_struct_parsing():
    cases = I.crafted_valid() + I.zlib_members()[:6]
    members = [I.frame(s, t, extra=b"ZZ\x03\0abc" if k % 3 == 1 else b"") for k, (_, s, t, _) in enumerate(cases)]
    blob, offs, sizes, out_offs = I.layout(members)
    rc, rows, crc, why = rows_of(blob, offs, sizes, out_offs)
    assert rc == 0 and not why.any()
    for k, m in enumerate(members):
        off, slen, want_crc, isize = I.parse(m)
        assert rows[k] == (int(offs[k]) + off, int(out_offs[k]), slen, isize) and crc[k] == want_crc
        assert blob[rows[k][0]:rows[k][0] + slen] == cases[k][1]
    assert rows_of(blob, offs, sizes, out_offs, why=False)[:2] == (0, rows)      # why_out may be NULL
    # the arrays mio_bgzf_scan fills give the same rows
    lib = F.load()
    o2, s2, oo2, w = np.zeros(64, np.int64), np.zeros(64, np.int32), np.zeros(65, np.int64), C.c_int32(0)
    buf = np.frombuffer(blob + b"\0" * 8, np.uint8)
    nb = lib.mio_bgzf_scan(buf.ctypes.data, len(blob), 64, 1 << 30, o2.ctypes.data, s2.ctypes.data, oo2.ctypes.data, C.addressof(w))
    assert nb == len(members)
    assert rows_of(blob, o2[:nb].copy(), s2[:nb].copy(), oo2[:nb + 1].copy())[1] == rows
    # the end marker: a member of no text
    blob, offs, sizes, out_offs = I.layout([cli.BGZF_EOF])
    rc, rows, crc, why = rows_of(blob, offs, sizes, out_offs)
    assert rc == 0 and rows == [(18, 0, 2, 0)] and crc[0] == 0 and why[0] == 0


def defect(name):
    good, _ = I.neighbour()
    m = bytearray(good)
    isize = None
    if name == "magic":
        m[1] = 0x8c
    elif name == "method":
        m[2] = 7
    elif name == "flags_fname":
        m[3] = 4 | 8
    elif name == "flags_none":
        m[3] = 0
    elif name == "xlen_past_member":
        m[10:12] = struct.pack("<H", len(m))
    elif name == "xlen_leaves_no_trailer":
        m[10:12] = struct.pack("<H", len(m) - 12 - 4)
    elif name == "no_bc":
        m[12:14] = b"XY"
    elif name == "bc_with_another_length":
        m[14:16] = struct.pack("<H", 3)
    elif name == "subfield_walks_past_xlen":
        m = bytearray(I.frame(bytes(good[18:-8]), b"", extra=b"ZZ\x40\0abc"))
        m[-8:] = good[-8:]
    elif name == "bsize_too_small":
        m[16:18] = struct.pack("<H", len(m) - 2)
    elif name == "bsize_too_large":
        m[16:18] = struct.pack("<H", len(m))
    elif name == "isize_not_out_offs":
        isize = struct.unpack_from("<I", m, len(m) - 4)[0] + 1
    elif name == "isize_above_65536":
        m[-4:] = struct.pack("<I", 65537)
        isize = 65537
    elif name == "shorter_than_a_member":
        m = m[:25]
    return bytes(m), isize


DEFECTS = ["magic", "method", "flags_fname", "flags_none", "xlen_past_member", "xlen_leaves_no_trailer", "no_bc",
           "bc_with_another_length", "subfield_walks_past_xlen", "bsize_too_small", "bsize_too_large", "isize_not_out_offs",
           "isize_above_65536", "shorter_than_a_member"]


@pytest.mark.parametrize("name", DEFECTS)
def test_a_header_defect_is_a_reason_never_an_error(name):
    good, _ = I.neighbour()
    bad, isize = defect(name)
    members = [good, bad, good]
    isizes = [struct.unpack_from("<I", m, len(m) - 4)[0] for m in members]
    if isize is not None:
        isizes[1] = isize
    blob, offs, sizes, out_offs = I.layout(members, isizes)
    rc, rows, crc, why = rows_of(blob, offs, sizes, out_offs)
    assert rc == 0
    assert why.tolist() == [I.OK, I.HEADER, I.OK]
    assert rows[1][3] == -1 and rows[0][3] == rows[2][3] == isizes[0] and rows[2][1] == int(out_offs[2])
    assert crc[0] == crc[2] == I.parse(good)[2]


def test_isize_65536_and_zero_are_taken():
    full = I.zlib_members()
    name, stream, text, _ = next(c for c in full if c[0] == "isize65536")
    blob, offs, sizes, out_offs = I.layout([I.frame(stream, text), cli.BGZF_EOF])
    rc, rows, crc, why = rows_of(blob, offs, sizes, out_offs)
    assert rc == 0 and not why.any() and rows[0][3] == 65536 and rows[1][3] == 0 and rows[1][1] == 65536


def test_argument_errors():
    good, _ = I.neighbour()
    blob, offs, sizes, out_offs = I.layout([good, good])
    lib = L.load()
    assert rows_of(blob, offs, sizes, out_offs)[0] == 0
    assert rows_of(blob, offs, sizes, out_offs, n=-1)[0] == L.E_INVALID
    assert rows_of(blob[:-1], offs, sizes, out_offs)[0] == L.E_INVALID                     # the last member ends outside `in`
    assert b"does not lie inside" in lib.mpb_last_error()
    assert rows_of(blob, offs - 1, sizes, out_offs)[0] == L.E_INVALID                      # a negative offset
    assert rows_of(blob, offs, -sizes, out_offs)[0] == L.E_INVALID
    assert rows_of(blob, offs, sizes, out_offs[::-1].copy())[0] == L.E_INVALID             # out_offs decreases
    assert b"decreases" in lib.mpb_last_error()
    assert rows_of(blob, offs, sizes, out_offs - 5)[0] == L.E_INVALID
    rows = (L.BgzfMemberRow * 2)()
    crc = np.zeros(2, np.uint32)
    buf = np.frombuffer(blob, np.uint8)
    args = [buf.ctypes.data, len(blob), offs.ctypes.data, sizes.ctypes.data, out_offs.ctypes.data, 2, C.addressof(rows), crc.ctypes.data, None]
    assert lib.mpb_bgzf_member_rows(*args) == 0
    for k in (0, 2, 3, 4, 6, 7):
        a = list(args)
        a[k] = None
        assert lib.mpb_bgzf_member_rows(*a) == L.E_INVALID, k
    assert lib.mpb_bgzf_member_rows(buf.ctypes.data, -1, *args[2:]) == L.E_INVALID
    assert lib.mpb_bgzf_member_rows(None, 0, None, None, out_offs.ctypes.data, 0, None, None, None) == 0      # no member at all
