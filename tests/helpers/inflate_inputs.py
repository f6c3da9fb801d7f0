"""Inputs shared by the tests of the device inflater (k_bgzf_inflate): the CPU model test of its lane code
(tests/test_inflate_lane_model.py), the rows test (tests/test_bgzf_member_rows.py) and the GPU test
(tests/test_gpu_bgzf_inflate.py).  Raw deflate streams come from zlib at chosen settings or from a small bit writer that emits
stored / fixed / dynamic blocks from a token list and chosen code lengths; frame() wraps a stream into a BGZF member.  Everything
is seeded and every member is at most 64 KiB each way."""
import functools
import struct
import zlib

import numpy as np

from helpers import bgzf_inputs as B

# MPB_BGZF_WHY_* (include/moira_pb.h)
(OK, HEADER, BLOCK_TYPE, STORED_LENGTH, CODE_LENGTH_CODE, REPEAT, TREE, SYMBOL, DISTANCE, OVERRUN, SHORT, TRUNCATED, TRAILING_BYTES,
 CRC) = range(14)

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
             12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 32
# a complete code over all 19 code-length symbols: 13 of 4 bits, 6 of 5 bits
CL_DEFAULT = [4] * 13 + [5] * 6
# a complete code over all 286 literal / length symbols: 226 of 8 bits, 60 of 9 bits
LL_FLAT = [8] * 226 + [9] * 60


def frame(stream, text, extra=b"", crc=None, isize=None, bc=True):
    """The BGZF member around a raw deflate stream that states `text`'s CRC-32 and length (or the given ones); `extra`: another
    subfield's bytes in front of 'B','C'; bc=False: no 'B','C' subfield at all (six other bytes in its place)."""
    xlen = len(extra) + 6
    bsize = 12 + xlen + len(stream) + 8 - 1
    assert bsize < 65536
    sub = b"BC\x02\0" + struct.pack("<H", bsize) if bc else b"XY\x02\0" + struct.pack("<H", bsize)
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff" + struct.pack("<H", xlen) + extra + sub + stream +
            struct.pack("<II", zlib.crc32(text) if crc is None else crc, len(text) if isize is None else isize))


def parse(member):
    """(stream offset, stream length, crc, isize) of a member by struct parsing (xlen read from the header)."""
    xlen, = struct.unpack_from("<H", member, 10)
    crc, isize = struct.unpack_from("<II", member, len(member) - 8)
    return 12 + xlen, len(member) - 12 - xlen - 8, crc, isize


class Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, value, nbits):                         # least significant bit first
        self.acc |= (value & ((1 << nbits) - 1)) << self.n
        self.n += nbits
        while self.n >= 8:
            self.out.append(self.acc & 0xff)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, nbits):                         # a Huffman code: most significant bit first
        self.put(int(format(code, "0%db" % nbits)[::-1], 2), nbits)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)

    def bytes(self):
        self.align()
        return bytes(self.out)


def canonical(lens):
    """{symbol: (code, length)} of the canonical code with these lengths (RFC 1951 3.2.2), whatever its Kraft sum."""
    count = [0] * 17
    for l in lens:
        count[l] += 1
    count[0] = 0
    code, nxt = 0, [0] * 17
    for l in range(1, 16):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = {}
    for s, l in enumerate(lens):
        if l:
            out[s] = (nxt[l] & ((1 << l) - 1), l)
            nxt[l] += 1
    return out


def put_tokens(w, tokens, ll, dd):
    """tokens: int (a literal) | ("m", length, distance) | ("ll", symbol) | ("d", symbol, extra bits, their count) -- the last two
    emit a bare symbol, for the invalid inputs.  Ends with the end-of-block code unless the last token is ("noeob",)."""
    for t in tokens:
        if isinstance(t, int):
            w.code(*ll[t])
        elif t[0] == "m":
            _, length, dist = t
            ls = max(k for k in range(29) if LEN_BASE[k] <= length) if length < 258 else 28
            w.code(*ll[257 + ls])
            w.put(length - LEN_BASE[ls], LEN_EXTRA[ls])
            ds = max(k for k in range(30) if DIST_BASE[k] <= dist)
            w.code(*dd[ds])
            w.put(dist - DIST_BASE[ds], DIST_EXTRA[ds])
        elif t[0] == "ll":
            w.code(*ll[t[1]])
        elif t[0] == "d":
            w.code(*dd[t[1]])
            w.put(t[2], t[3])
    if not (tokens and tokens[-1] == ("noeob",)):
        w.code(*ll[256])


def stored_block(w, data, final, nlen=None, length=None):
    w.put(1 if final else 0, 1)
    w.put(0, 2)
    w.align()
    n = len(data) if length is None else length
    w.put(n, 16)
    w.put((~n & 0xffff) if nlen is None else nlen, 16)
    for b in data:
        w.put(b, 8)


def fixed_block(w, tokens, final):
    w.put(1 if final else 0, 1)
    w.put(1, 2)
    put_tokens(w, tokens, canonical(FIXED_LL), canonical(FIXED_D))


def dynamic_block(w, tokens, ll_lens, d_lens, final, cl_lens=None, seq=None, hlit=None, hdist=None):
    """A dynamic block whose code lengths are sent one by one (no repeat codes) unless `seq` gives the code-length symbols as
    [(symbol, extra value)]; `cl_lens`: the 19 lengths of the code-length code."""
    cl_lens = CL_DEFAULT if cl_lens is None else cl_lens
    w.put(1 if final else 0, 1)
    w.put(2, 2)
    w.put((len(ll_lens) if hlit is None else hlit) - 257, 5)
    w.put((len(d_lens) if hdist is None else hdist) - 1, 5)
    w.put(19 - 4, 4)
    for s in CL_ORDER:
        w.put(cl_lens[s], 3)
    cl = canonical(cl_lens)
    if seq is None:
        seq = [(l, 0) for l in list(ll_lens) + list(d_lens)]
    for sym, extra in seq:
        w.code(*cl[sym])
        if sym >= 16:
            w.put(extra, {16: 2, 17: 3, 18: 7}[sym])
    if tokens is not None:
        put_tokens(w, tokens, canonical(ll_lens), canonical(d_lens))


def text_of(tokens, before=b""):
    out = bytearray(before)
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        elif t[0] == "m":
            for _ in range(t[1]):
                out.append(out[-t[2]])
    return bytes(out[len(before):])


def deflate(text, level=6, mem=8, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, mem, strategy)
    return c.compress(text) + c.flush()


def fibonacci_text():
    """22 byte values with Fibonacci counts (46,367 bytes), shuffled: Z_HUFFMAN_ONLY gives them literal codes of up to 15 bits."""
    fib = [1, 1]
    while len(fib) < 22:
        fib.append(fib[-1] + fib[-2])
    a = np.concatenate([np.full(c, 65 + k, np.uint8) for k, c in enumerate(fib)])
    np.random.default_rng(7).shuffle(a)
    assert len(a) == 46367
    return a.tobytes()


@functools.lru_cache(None)
def zlib_members():
    """[(name, stream, text, expected blocks or None)] from zlib's settings; blocks = (stored, fixed, dynamic)."""
    rng = np.random.default_rng(11)
    t = B.fastq_like(rng, B.DATA)
    out = [("level%d" % lv, deflate(t, lv), t, (0, 0, 1)) for lv in (1, 4, 9)]
    out.append(("memlevel1", deflate(t, 6, 1), t, None))
    out.append(("fixed", deflate(t, 6, 8, zlib.Z_FIXED), t, (0, 1, 0)))
    out.append(("level0", deflate(t, 0), t, (2, 0, 0)))
    out.append(("rle", deflate(t, 6, 8, zlib.Z_RLE), t, None))
    fib = fibonacci_text()
    out.append(("fibonacci", deflate(fib, 6, 8, zlib.Z_HUFFMAN_ONLY), fib, None))
    full = B.fastq_like(np.random.default_rng(12), 65536)
    out.append(("isize65536", deflate(full, 6), full, None))
    for name, text in B.named_inputs():
        for k, m in enumerate(B.members(text)):
            s = deflate(m, 6)
            if len(s) < 65000:
                out.append(("%s_%d" % (name, k), s, m, None))
    for r, text in enumerate(B.golden_renderings()):
        for k, m in enumerate(B.members(text)[:2]):
            out.append(("golden%d_%d" % (r, k), deflate(m, 4), m, None))
    return out


@functools.lru_cache(None)
def fuzz_members(count=24):
    """[(name, stream, text, None)]: bgzf_inputs' fuzz members, each at a random level / memLevel / strategy."""
    out = []
    for k in range(count):
        rng = np.random.default_rng(500 + k)
        text = B.fuzz_member(k)
        level, mem = int(rng.integers(0, 10)), int(rng.integers(1, 10))
        strategy = [zlib.Z_DEFAULT_STRATEGY, zlib.Z_FILTERED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE, zlib.Z_FIXED][int(rng.integers(0, 5))]
        s = deflate(text, level, mem, strategy)
        if len(s) >= 65000:                              # (a stored rendering of a long random member: what fits the size field)
            text = text[:60000]
            s = deflate(text, level, mem, strategy)
        out.append(("fuzz%d" % k, s, text, None))
    return out


def _dist_ladder():
    """Distance code lengths 1, 2, ..., 14, 15, 15 (16 symbols); the two 15-bit codes are symbols 14 and 15 (distances 129..256)."""
    return list(range(1, 15)) + [15, 15]


@functools.lru_cache(None)
def crafted_valid():
    """[(name, stream, text, blocks)] from the bit writer."""
    rng = np.random.default_rng(21)
    out = []
    lead = rng.integers(65, 91, 300).tolist()

    def one(name, build, blocks=None):
        w = Bits()
        text = build(w)
        out.append((name, w.bytes(), text, blocks))

    def ladder(w):
        toks = lead + [("m", 10, 130), ("m", 20, 200), ("m", 3, 1), ("m", 258, 256), 66, ("m", 5, 193)]
        dynamic_block(w, toks, LL_FLAT, _dist_ladder(), True)
        return text_of(toks)
    one("dist_ladder_15bit", ladder, (0, 0, 1))

    def one_dist(w):
        toks = [65, 66, ("m", 30, 1), 67, ("m", 258, 1)]
        dynamic_block(w, toks, LL_FLAT, [1], True)
        return text_of(toks)
    one("single_1bit_distance_code", one_dist, (0, 0, 1))

    def no_dist(w):
        toks = lead[:50]
        dynamic_block(w, toks, LL_FLAT, [0], True)
        return text_of(toks)
    one("literal_only_hdist1_len0", no_dist, (0, 0, 1))

    def empty_stored(w):
        stored_block(w, bytes(lead[:40]), False)
        stored_block(w, b"", False)
        toks = [("m", 40, 40), 90]
        fixed_block(w, toks, True)
        return bytes(lead[:40]) + text_of(toks, bytes(lead[:40]))
    one("empty_stored_between", empty_stored, (2, 1, 0))

    def run258(w):
        toks = [88, ("m", 258, 1)]
        fixed_block(w, toks, True)
        return text_of(toks)
    one("match258_distance1", run258, (0, 1, 0))

    def far(w):
        first = rng.integers(0, 256, 32768).astype(np.uint8).tobytes()
        stored_block(w, first, False)
        toks = [("m", 258, 32768), ("m", 3, 32768)]
        fixed_block(w, toks, True)
        return first + text_of(toks, first)
    one("match_distance32768_ends_on_last_byte", far, (1, 1, 0))

    def end_marker(w):
        fixed_block(w, [], True)
        return b""
    one("end_marker", end_marker, (0, 1, 0))

    def repeats(w):
        # zero runs by repeat code 18 (65, 138 and 50 zeros) around four 2-bit codes: A, B, C and end-of-block (HLIT 257)
        toks = [65, 66, 67]
        ll = [0] * 65 + [2, 2, 2] + [0] * 188 + [2]
        seq = [(18, 54), (2, 0), (2, 0), (2, 0), (18, 138 - 11), (18, 50 - 11), (2, 0), (0, 0)]
        dynamic_block(w, toks, ll, [0], True, seq=seq)
        return text_of(toks)
    one("repeat_code_18", repeats, (0, 0, 1))
    return out


@functools.lru_cache(None)
def crafted_invalid():
    """[(name, member, why)]: one whole member per reason the device hands a member back.  `member` states the CRC and length of the
    text the stream would make if it were accepted as far as it goes."""
    rng = np.random.default_rng(31)
    lits = rng.integers(65, 91, 40).tolist()
    text = bytes(lits)
    out = []

    def add(name, why, build, stated=None, **kw):
        w = Bits()
        build(w)
        out.append((name, frame(w.bytes(), text if stated is None else stated, **kw), why))

    def btype3(w):
        w.put(1, 1); w.put(3, 2)
    add("btype3", BLOCK_TYPE, btype3)
    add("len_not_nlen", STORED_LENGTH, lambda w: stored_block(w, text, True, nlen=0x1234))
    add("stored_longer_than_stream", TRUNCATED, lambda w: stored_block(w, text[:20], True, length=40))
    over_cl = [4] * 13 + [5] * 5 + [4]                                  # Kraft sum above 1
    under_cl = [4] * 13 + [5] * 5 + [6]                                 # ... below 1
    add("cl_oversubscribed", CODE_LENGTH_CODE, lambda w: dynamic_block(w, lits, LL_FLAT, [1], True, cl_lens=over_cl))
    add("cl_incomplete", CODE_LENGTH_CODE, lambda w: dynamic_block(w, lits, LL_FLAT, [1], True, cl_lens=under_cl))
    add("repeat16_first", REPEAT, lambda w: dynamic_block(w, None, LL_FLAT, [1], True, seq=[(16, 0)]))
    add("repeat_past_total", REPEAT,
        lambda w: dynamic_block(w, None, LL_FLAT, [1], True, seq=[(l, 0) for l in LL_FLAT] + [(18, 127)]))
    ll_over = [8] * 227 + [9] * 59
    ll_under = [8] * 225 + [9] * 61
    add("lit_tree_oversubscribed", TREE, lambda w: dynamic_block(w, None, ll_over, [1], True))
    add("lit_tree_incomplete", TREE, lambda w: dynamic_block(w, None, ll_under, [1], True))
    add("dist_tree_oversubscribed", TREE, lambda w: dynamic_block(w, None, LL_FLAT, [1, 1, 1], True))
    add("dist_tree_incomplete", TREE, lambda w: dynamic_block(w, None, LL_FLAT, [2, 2, 2], True))
    no_eob = [8] * 256 + [0]                                            # complete without symbol 256 (HLIT 257)
    add("no_end_of_block_code", TREE, lambda w: dynamic_block(w, None, no_eob, [1], True))
    add("symbol286_fixed", SYMBOL, lambda w: fixed_block(w, lits + [("ll", 286), ("noeob",)], True))
    add("distance_symbol30", DISTANCE, lambda w: fixed_block(w, lits + [("ll", 257), ("d", 30, 0, 0), ("noeob",)], True))
    add("distance_before_start", DISTANCE, lambda w: fixed_block(w, lits[:5] + [("m", 3, 6)], True), stated=text_of(lits[:5]) + b"AAA")
    add("literal_past_isize", OVERRUN, lambda w: fixed_block(w, lits + [65], True))
    add("match_crossing_isize", OVERRUN, lambda w: fixed_block(w, lits[:38] + [("m", 3, 10)], True))
    add("final_block_one_short", SHORT, lambda w: fixed_block(w, lits[:39], True))
    add("trailing_byte", TRAILING_BYTES, lambda w: (fixed_block(w, lits, True), w.align(), w.put(0, 8)))
    # a zlib stream cut inside a symbol: the last two bytes of a dynamic block are gone
    t = B.fastq_like(np.random.default_rng(32), 3000)
    out.append(("cut_mid_symbol", frame(deflate(t, 6)[:-2], t), TRUNCATED))
    good = Bits()
    fixed_block(good, lits, True)
    out.append(("wrong_crc", frame(good.bytes(), text, crc=zlib.crc32(text) ^ 1), CRC))
    out.append(("wrong_isize", frame(good.bytes(), text, isize=len(text) + 1), SHORT))
    out.append(("no_bc_subfield", frame(good.bytes(), text, bc=False), HEADER))
    return out


def neighbour():
    """A small valid member to put on either side of an invalid one."""
    t = b"@r\nACGTACGTACGTACGT\n+\nIIIIIIIIIIIIIIII\n" * 20
    return frame(deflate(t, 6), t), t


def layout(members, isizes=None):
    """(blob, offs, sizes, out_offs) of members laid back to back, as mio_bgzf_scan would fill them (ISIZE from each trailer)."""
    blob = b"".join(members)
    sizes = np.array([len(m) for m in members], np.int32)
    offs = np.concatenate([[0], np.cumsum(sizes[:-1], dtype=np.int64)]).astype(np.int64)
    isz = [struct.unpack_from("<I", m, len(m) - 4)[0] for m in members] if isizes is None else isizes
    out_offs = np.concatenate([[0], np.cumsum(isz, dtype=np.int64)]).astype(np.int64)
    return blob, offs, sizes, out_offs


def host_inflate(members):
    """(text or None, error or None) per member from libmoira_io's mio_bgzf_inflate_mt, each member on its own."""
    from moira_amd import fastio
    L = fastio.load()
    res = []
    for m in members:
        blob, offs, sizes, out_offs = layout([m])
        out = np.zeros(max(int(out_offs[1]), 1), np.uint8)
        buf = np.frombuffer(blob + b"\0" * 8, np.uint8)
        rc = L.mio_bgzf_inflate_mt(buf.ctypes.data, offs.ctypes.data, sizes.ctypes.data, out_offs.ctypes.data, 1, out.ctypes.data, 1)
        res.append((None, L.mio_inflate_error().decode()) if rc < 0 else (out[:int(out_offs[1])].tobytes(), None))
    return res
