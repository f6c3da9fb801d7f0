"""Host-side mirror of the reference's filter path, batch-shaped.

Reference interface mirrored (same argument meaning and error behaviour):
  * `bernoulli.calculate_errors_PB(contig, contig_quals, alpha)`  moira/bernoullimodule.c:66-114
  * the filter half of `process_data`                             moira/moira.py:806-831
  * the keep/discard predicate of `write_results`                 moira/moira.py:911,925-926,949-950
What replaces moira's per-read `Pool.apply_async` dispatch (moira/moira.py:431-454) is:
pack a chunk of reads into an (N x L_max) uint8 matrix -> one library call -> arrays back.

Everything is computed by libmoira_pb.so on the GPU; this module only marshals.
"""
import ctypes as C
import math

import numpy as np

from . import _lib as L


def _round_up(x, m):
    return (x + m - 1) // m * m


class DeviceBuffer:
    """A device allocation owned by an Engine (freed with it or by .free())."""

    def __init__(self, engine, nbytes):
        self.engine, self.nbytes = engine, int(nbytes)
        p = C.c_void_p()
        L.check(engine.lib.mpb_malloc(engine.ctx, self.nbytes, C.byref(p)))
        self.ptr = p.value

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.nbytes
        L.check(self.engine.lib.mpb_memcpy_h2d(self.engine.ctx, self.ptr, arr.ctypes.data, arr.nbytes))
        return self

    def download(self, dtype, count, offset=0):
        """`count` items of `dtype` starting `offset` BYTES into the allocation."""
        out = np.empty(count, dtype)
        assert offset >= 0 and offset + out.nbytes <= self.nbytes
        L.check(self.engine.lib.mpb_memcpy_d2h(self.engine.ctx, out.ctypes.data, self.ptr + int(offset), out.nbytes))
        return out

    def free(self):
        if self.ptr:
            L.check(self.engine.lib.mpb_free(self.engine.ctx, self.ptr))
            self.ptr = None


class FilterResult:
    """Per-read outputs of one batch: ee (after +Ns / floor, i.e. what process_data returns),
    ns, passed (bool) and the batch totals."""

    def __init__(self, ee, ns, passed, n_pass, n_overflow):
        self.ee, self.ns, self.passed = ee, ns, passed
        self.n_pass, self.n_fail, self.n_overflow = n_pass, len(ee) - n_pass, n_overflow


class TextFilterResult(FilterResult):
    """FilterResult of Engine.filter_text, with what the device pack produced next to it: lens (bases packed per read) and
    has_n (an upper-case 'N' among them)."""

    def __init__(self, ee, ns, passed, lens, has_n, n_pass, n_overflow):
        FilterResult.__init__(self, ee, ns, passed, n_pass, n_overflow)
        self.lens, self.has_n = lens, has_n


class NotTaken(Exception):
    """The device did not take a text for indexing (Engine.fastq_index, Engine.filter_fastq): .why is MPB_FQ_WHY_* (1 a byte
    >= 0x80, 2 a lone carriage return, 3 the line table would not fit, 4 a row check failed), str() names it.  The caller
    indexes on the host (fastio.index), which raises whatever there is to raise.  .which: the text it speaks of where a call takes
    two (Engine.contigs_filter_fastq: 0 forward, 1 reverse; Engine.fasta_qual_index, Engine.filter_fasta_qual: 0 fasta, 1 qual,
    with MPB_FA_WHY_* beside the four reasons above -- names: _lib.FA_WHY), else None.  .bad_record: the first offending record
    where the device named one, else None."""

    def __init__(self, why, which=None, bad_record=None):
        Exception.__init__(self, L.FA_WHY[why] if 0 <= why < len(L.FA_WHY) else "reason %d" % why)
        self.why, self.which, self.bad_record = why, which, bad_record


class FastaQualFilterResult(TextFilterResult):
    """TextFilterResult of Engine.filter_fasta_qual, with what the device built of the two texts next to it: .text (a uint8
    array: the slots header | sequence | one byte per quality), .idx (the record index over it), .f_consumed and .q_consumed
    as fastio.fasta_qual_index returns them.  .resident: the generation of the slots and index the call left on the device."""

    def __init__(self, text, idx, f_consumed, q_consumed, *a):
        TextFilterResult.__init__(self, *a)
        self.text, self.idx, self.f_consumed, self.q_consumed = text, idx, f_consumed, q_consumed
        self.resident = 0


class FastqFilterResult(TextFilterResult):
    """TextFilterResult of Engine.filter_fastq, with the record index the device built next to it: idx, consumed, bad as
    fastio.index returns them.  .resident: the generation of the text and index the call left on the device
    (Engine.format_text(resident=...)); 0 when there is none."""

    def __init__(self, idx, consumed, bad, *a):
        TextFilterResult.__init__(self, *a)
        self.idx, self.consumed, self.bad = idx, consumed, bad
        self.resident = 0


class NotResident(Exception):
    """Engine.format_text(resident=g): g is not the generation of the text the context holds -- a later call of filter_fastq,
    filter_bgzf_fastq, fastq_index, contigs_filter_fastq, fasta_qual_index or filter_fasta_qual has replaced or dropped it.  Nothing was touched: the caller formats
    on the host (fastio.format_records) or from an upload."""


class MembersNotTaken(Exception):
    """Engine.filter_bgzf_fastq handed a batch back because of one of its members: .first is the lowest member that was not
    taken, .done (uint8 per member) is 1 where the device took the member and its CRC-32 matched, .why (uint8 per member) is
    MPB_BGZF_WHY_* (names: _lib.BGZF_WHY).  Nothing was filtered: the caller inflates the batch on the host, whose decoder raises
    whatever there is to raise, and goes on through Engine.filter_fastq."""

    def __init__(self, first, done, why):
        w = int(why[first])
        Exception.__init__(self, "member %d: %s" % (first, L.BGZF_WHY[w] if 0 <= w < len(L.BGZF_WHY) else "reason %d" % w))
        self.first, self.done, self.why = first, done, why


class BgzfFastqFilterResult(FastqFilterResult):
    """FastqFilterResult of Engine.filter_bgzf_fastq, with .text (a uint8 array: the carry followed by the inflated members, or
    None when the caller did not ask for it) and .member_stats (the call's mpb_bgzf_inflate_stats as a dict)."""

    def __init__(self, text, member_stats, *a):
        FastqFilterResult.__init__(self, *a)
        self.text, self.member_stats = text, member_stats


TEXT_ROW_DTYPE = np.dtype([("seq_off", "<i8"), ("qual_off", "<i8"), ("len", "<i4"), ("pad", "<i4")])     # mpb_text_row


def _text_ptr(buf):
    """A chunk of text (bytes, bytearray, memoryview or a uint8 array) -> (object to keep alive, address, length)."""
    if isinstance(buf, np.ndarray):
        a = np.ascontiguousarray(buf).view(np.uint8).reshape(-1)
    else:
        a = np.frombuffer(buf, np.uint8)
    return a, a.ctypes.data, int(a.size)


def _index_args(idx, sel):
    idx = np.ascontiguousarray(idx, np.int64)
    if idx.ndim != 2 or idx.shape[1] != 6:
        raise ValueError("idx must be an (n_records x 6) int64 record index")
    if sel is not None:
        sel = np.ascontiguousarray(sel, np.int64).reshape(-1)
    return idx, sel, (len(sel) if sel is not None else len(idx))


def _check_text(rc, bad):
    try:
        L.check(rc)
    except ValueError as e:
        e.bad_record = bad.value
        raise


def _record_error(buf, idx, n, kind):
    """fastio.index's third value from a device-built index: None, or the RecordError of row n (.row: its six columns; the
    header is None where the caller holds no text)."""
    if not kind:
        return None
    from . import fastio
    err = fastio.RecordError(kind, fastio.header_of(buf, idx[n]) if buf is not None else None)
    err.row = idx[n].copy()
    return err


def _filter_error(frc, fbad):
    """What a fused call's filter refused, as the ValueError filter_text would have raised (.bad_record), or None."""
    try:
        _check_text(frc.value, fbad)
    except ValueError as e:
        return e


def _record_limit(max_records):
    """max_records as the text-alone entries take it (None: no limit)."""
    limit = (1 << 62) if max_records is None else int(max_records)
    if limit < 0:
        raise ValueError("max_records must not be negative")
    return limit


def _contig_params(match, mismatch, gap, insert, deltaq, consensus, qscore_cap, trim_overlap):
    return L.ContigParams(int(match), int(mismatch), int(gap), int(insert), int(deltaq), int(consensus), int(qscore_cap),
                          1 if trim_overlap else 0)


class _TextResults:
    """The five per-record result arrays of a text entry -- ee, ns, pass, lens, flags -- for `n` records: fresh, or the
    caller's own (`out`)."""
    DTYPES = (np.float64, np.int32, np.uint8, np.int32, np.uint8)

    def __init__(self, n, out=None):
        if out is None:
            out = tuple(np.empty(n, t) for t in self.DTYPES)
        ee, ns, ps, lens, flags = out
        if (ee.dtype, ns.dtype, ps.dtype, lens.dtype, flags.dtype) != self.DTYPES or \
                not all(a.flags.c_contiguous and len(a) >= n for a in out):
            raise ValueError("out must be contiguous (float64, int32, uint8, int32, uint8) arrays of at least n entries")
        self.arrays = ee, ns, ps, lens, flags

    def ptrs(self):
        return tuple(a.ctypes.data for a in self.arrays)

    def cut(self, n):
        """-> (ee, ns, passed, lens, has_n) of the first n records (pass and flag bytes are 0 / 1)."""
        ee, ns, ps, lens, flags = (a[:n] for a in self.arrays)
        return ee, ns, ps.view(bool), lens, flags.view(bool)


def _ask_again(call, cap, limit, out_cap=None, grow_out=False):
    """The capacity loop of the text-alone entries.  call(cap, out_cap) makes one call of the entry with room for `cap` index
    rows (and `out_cap` bytes of output, where the entry has such a capacity) and returns (rc, the rows it needs, the bytes it
    needs or None).  An entry that ended in MPB_E_INVALID because it counted more rows than the guess is asked once more with
    their number -- never above limit + 1 rows -- and with 16 bytes more of output per row where grow_out says the byte
    capacity was a guess as well; one that needs more bytes is asked again with them.  -> (the last rc, the calls made)."""
    calls = 0
    while True:
        calls += 1
        rc, rows, nbytes = call(cap, out_cap)
        if rc == L.E_INVALID and rows > cap and cap < limit + 1:
            if grow_out:
                out_cap += 16 * (rows - cap)
            cap = rows                                       # the text holds more records than the guess: their number is known now
            continue
        if rc == L.E_INVALID and nbytes is not None and nbytes > out_cap:
            out_cap = nbytes
            continue
        return rc, calls


def text_rows(idx, sel=None, text_bytes=0, max_len=0, stride=0):
    """The validated row descriptors (mpb_text_rows; host only) of the records sel (None: all) of the record index idx over a
    text of text_bytes bytes -> (rows, longest): rows a TEXT_ROW_DTYPE array (None when stride == 0: validation and the
    longest packed length only).  ValueError (MPB_E_INVALID) for an offset or length the text cannot hold, a sel entry outside
    the index, a read above 65535 bases or above the stride; .bad_record = its position in sel order."""
    idx, sel, n = _index_args(idx, sel)
    rows = np.zeros(n, TEXT_ROW_DTYPE) if stride else None
    longest, bad = C.c_int64(0), C.c_int64(-1)
    rc = L.load().mpb_text_rows(idx.ctypes.data if len(idx) else None, len(idx), sel.ctypes.data if sel is not None else None, n,
                                int(text_bytes), int(max_len), int(stride), rows.ctypes.data if rows is not None else None,
                                C.byref(longest), C.byref(bad))
    _check_text(rc, bad)
    return rows, longest.value


PAIR_ROW_DTYPE = np.dtype([("fseq_off", "<i8"), ("fqual_off", "<i8"), ("fhdr_off", "<i8"), ("rseq_off", "<i8"), ("rqual_off", "<i8"),
                           ("l1", "<i4"), ("l2", "<i4"), ("hdr_len", "<i4"), ("pad", "<i4")])     # mpb_pair_row


def pair_rows(fidx, ridx, ftext_bytes, rtext_bytes, rec_cap):
    """The validated pair descriptors (mpb_pair_rows; host only) of the two record indexes over texts of the given sizes -> a
    PAIR_ROW_DTYPE array.  ValueError (MPB_E_INVALID) for an offset or length outside its text, a sequence and quality line
    of different lengths, or hdr_len + 2 (l1 + l2) > rec_cap; .bad_record = the pair's position."""
    fidx, ridx = np.ascontiguousarray(fidx, np.int64), np.ascontiguousarray(ridx, np.int64)
    if fidx.ndim != 2 or fidx.shape[1] != 6 or fidx.shape != ridx.shape:
        raise ValueError("fidx and ridx must be (n x 6) int64 record indexes of the same length")
    rows = np.zeros(len(fidx), PAIR_ROW_DTYPE)
    bad = C.c_int64(-1)
    rc = L.load().mpb_pair_rows(fidx.ctypes.data, ridx.ctypes.data, len(fidx), int(ftext_bytes), int(rtext_bytes), int(rec_cap),
                                rows.ctypes.data, C.byref(bad))
    _check_text(rc, bad)
    return rows


class ContigResult:
    """What Engine.contigs_text returns (see there)."""
    __slots__ = ("cbuf", "cidx", "aux", "done", "rec_cap", "n_done", "n_handed_back", "aln", "aln_len", "score")

    def __init__(self, *a):
        for k, v in zip(self.__slots__, a):
            setattr(self, k, v)


class ContigFilterResult(ContigResult):
    """What Engine.contigs_filter_text returns: ContigResult's fields, and the filter's results where the contigs lie -- ee, ns,
    passed, lens, has_n per pair (defined where filtered is True), n_pass / n_overflow over the filtered pairs, and filter_error:
    None, or the ValueError Engine.filter_text would have raised over the built pairs (.bad_record), not raised."""
    __slots__ = ("ee", "ns", "passed", "lens", "has_n", "filtered", "n_pass", "n_overflow", "filter_error")

    def __init__(self, contigs, *a):
        for k in ContigResult.__slots__:
            setattr(self, k, getattr(contigs, k))
        for k, v in zip(ContigFilterResult.__slots__, a):
            setattr(self, k, v)


class PairedFastqResult(ContigFilterResult):
    """What Engine.contigs_filter_fastq returns: ContigFilterResult's fields over the n_built pairs, and what the device made of
    the two texts -- fidx / ridx, f_bad / r_bad as fastio.index(text, final, max_records) returns them for each file, n_pairs
    (min of the two record counts), mismatch (fastio.first_header_mismatch over n_pairs pairs, or -1), n_built (the pairs the
    contigs were built for: mismatch < 0 ? n_pairs : mismatch), f_consumed / r_consumed (what fastio.index(text, final, n_pairs)
    consumes), calls (how often the entry was asked: 1 + the capacities that had to be asked for again) and resident: the
    generation of the contigs the call left on the device (cbuf, cidx and aux where they lie: Engine.format_text / format_report /
    collapse_text take it), or 0 -- a handed-back pair or a refused filter leaves none."""
    __slots__ = ("fidx", "ridx", "f_consumed", "r_consumed", "f_bad", "r_bad", "mismatch", "n_pairs", "n_built", "calls", "resident")

    def __init__(self, res, *a):
        for k in ContigResult.__slots__ + ContigFilterResult.__slots__:
            setattr(self, k, getattr(res, k))
        for k, v in zip(PairedFastqResult.__slots__, a):
            setattr(self, k, v)


def check_host_batch(q, lens, fixed_len, out, limit):
    """Argument checks shared by every host-batch entry (one GPU or several): -> (q, n, stride, lens, (ee, ns, ps)).
    `limit`: longest read the method takes (None: as long as the row)."""
    q = np.ascontiguousarray(q, dtype=np.uint8)
    if q.ndim != 2:
        raise ValueError("q must be a 2-D (reads x stride) uint8 matrix")
    n, stride = q.shape
    if lens is not None:
        lens = np.ascontiguousarray(lens, dtype=np.int32)
        if lens.shape != (n,):
            raise ValueError("lens must have one entry per read")
        if n and (lens.min() < 0 or lens.max() > stride):
            raise ValueError("a length does not fit the row stride")
        if n and limit is not None and lens.max() > limit:
            raise ValueError("reads longer than %d bases are not supported (longest: %d)" % (limit, int(lens.max())))
    elif fixed_len is None:
        raise ValueError("give lens or fixed_len")
    if out is None:
        res = np.empty(n, np.float64), np.empty(n, np.int32), np.empty(n, np.uint8)
    else:                                   # caller-owned result arrays (a streaming caller reuses them: fresh
        ee, ns, ps = out                    # arrays cost a page fault per 4 KiB, ~3 ms per 100 MB of results)
        if (ee.dtype, ns.dtype, ps.dtype) != (np.float64, np.int32, np.uint8) or \
                not (len(ee) >= n and len(ns) >= n and len(ps) >= n) or \
                not (ee.flags.c_contiguous and ns.flags.c_contiguous and ps.flags.c_contiguous):
            raise ValueError("out must be contiguous (float64, int32, uint8) arrays of at least n entries")
        res = ee[:n], ns[:n], ps[:n]
    return q, n, stride, lens, res


class Engine:
    """One context on one MI355X (one per process/rank; not thread-safe)."""

    batched_only = False      # True: never take the one-read-per-wave path for small batches (tests, diagnostics)

    def __init__(self, device=0):
        self.lib = L.load()
        ctx = C.c_void_p()
        L.check(self.lib.mpb_create(int(device), C.byref(ctx)))
        self.ctx = ctx
        self.device = int(device)
        self._pinned = {}

    def close(self):
        if getattr(self, "ctx", None):
            for p in list(getattr(self, "_pinned", {}).values()):
                self.lib.mpb_host_free(self.ctx, p)
            self._pinned = {}
            self.lib.mpb_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ---- parameters -------------------------------------------------------------------------
    @staticmethod
    def params(alpha=0.005, uncert=0.01, maxerrors=None, ambigs="treat_as_errors", round_=False,
               fast_fma=False, test_underpredict=False, decision_only=False, batched_only=False, count_cells=False,
               no_narrow=False, narrow_rows=0, narrow_split=0, odds=False, odds_narrow=False, poisson_device_tail=False):
        if ambigs not in L.AMBIG:
            raise ValueError("ambigs must be one of %s" % sorted(L.AMBIG))
        if odds and fast_fma:
            raise ValueError("odds and fast_fma are two arithmetics for the same pass: set one")
        if odds_narrow and not odds:
            raise ValueError("odds_narrow needs odds=True (MPB_FLAG_ODDS_NARROW needs MPB_FLAG_ODDS)")
        flags = (L.FLAG_ROUND if round_ else 0) | (L.FLAG_FAST_FMA if fast_fma else 0) | \
                (L.FLAG_TEST_UNDERPREDICT if test_underpredict else 0) | \
                (L.FLAG_DECISION_ONLY if decision_only else 0) | \
                (L.FLAG_BATCHED_ONLY if batched_only else 0) | (L.FLAG_COUNT_CELLS if count_cells else 0) | \
                (L.FLAG_NO_NARROW if no_narrow else 0) | (L.FLAG_ODDS if odds else 0) | \
                (L.FLAG_ODDS_NARROW if odds_narrow else 0) | (L.FLAG_POISSON_DEVICE_TAIL if poisson_device_tail else 0) | \
                L.FLAG_NARROW_ROWS(narrow_rows) | ((int(narrow_split) & 255) << 12)
        return L.FilterParams(float(alpha), float(uncert),
                              math.nan if maxerrors is None else float(maxerrors),
                              L.AMBIG[ambigs], flags)

    # ---- memory -----------------------------------------------------------------------------
    def alloc(self, nbytes):
        return DeviceBuffer(self, nbytes)

    def host_alloc(self, shape, dtype=np.uint8):
        """A numpy array over PINNED host memory (mpb_host_alloc): `filter()` DMA-s such a batch from where it
        lies instead of staging it.  Release it with host_free() (or with the engine)."""
        shape = (int(shape),) if np.isscalar(shape) else tuple(int(x) for x in shape)
        dt = np.dtype(dtype)
        nbytes = int(np.prod(shape)) * dt.itemsize
        p = C.c_void_p()
        L.check(self.lib.mpb_host_alloc(self.ctx, nbytes, C.byref(p)))
        buf = (C.c_uint8 * max(nbytes, 1)).from_address(p.value)
        arr = np.frombuffer(buf, dtype=dt, count=int(np.prod(shape))).reshape(shape)
        self._pinned[arr.ctypes.data] = p.value
        return arr

    def host_free(self, arr):
        p = self._pinned.pop(arr.ctypes.data, None)
        if p is not None and self.ctx:
            L.check(self.lib.mpb_host_free(self.ctx, p))

    def synchronize(self):
        L.check(self.lib.mpb_synchronize(self.ctx))

    def stream(self):
        p = C.c_void_p()
        L.check(self.lib.mpb_stream(self.ctx, C.byref(p)))
        return p.value

    # ---- packing ----------------------------------------------------------------------------
    def pack(self, seqs, quals, stride=None):
        """[(seq str|None)], [list[int]] -> (q uint8[n, stride], lens int32[n]).
        Q0 -> 1, 'N' -> 0, 'n' -> 255 (see include/moira_pb.h)."""
        n = len(quals)
        lens = np.array([len(x) for x in quals], np.int32)
        if stride is None:
            stride = _round_up(max(int(lens.max()) if n else 1, 1), 16)
        q = np.zeros((n, stride), np.uint8)
        for i in range(n):
            qi = np.ascontiguousarray(quals[i], dtype=np.int32)
            s = seqs[i] if seqs is not None else None
            if s is not None:
                if len(s) != len(qi):
                    raise ValueError("contig and contig_quals must have the same length")
                s = s.encode() if isinstance(s, str) else s
            L.check(self.lib.mpb_pack_read(s, qi.ctypes.data, len(qi), q[i].ctypes.data, stride))
        return q, lens

    def pack_batch_ascii(self, seqs, qual_strs, fastq_offset=33, stride=None, max_len=0):
        """Reads with raw FASTQ quality strings -> (q uint8[n, stride], lens): one C loop."""
        n = len(qual_strs)
        off = np.zeros(n + 1, np.int64)
        if n:
            off[1:] = np.cumsum([len(x) for x in qual_strs])
        lens_full = off[1:] - off[:-1]
        longest = int(min(lens_full.max(), max_len) if (n and max_len > 0) else (lens_full.max() if n else 1))
        if stride is None:
            stride = _round_up(max(longest, 1), 16)
        q = np.empty((n, stride), np.uint8)
        lens = np.empty(n, np.int32)
        if seqs is not None and any(len(s) != len(x) for s, x in zip(seqs, qual_strs)):
            raise ValueError("contig and contig_quals must have the same length")
        L.check(self.lib.mpb_pack_batch_ascii("".join(seqs).encode() if seqs is not None else None,
                                              "".join(qual_strs).encode("latin-1"), off.ctypes.data, n,
                                              int(fastq_offset), int(max_len), stride, q.ctypes.data,
                                              lens.ctypes.data))
        return q, lens

    # ---- FASTQ text as it lies in the file (mpb_text_rows, k_pack_text) ---------------------------
    @staticmethod
    def text_rows(idx, sel=None, text_bytes=0, max_len=0, stride=0):
        """The validated row descriptors of k_pack_text: see the module's text_rows (host only, needs no device)."""
        return text_rows(idx, sel, text_bytes, max_len, stride)

    def pack_text_device(self, d_text, text_bytes, d_rows, n, stride, d_q_out, d_len_out, d_flags_out=None, d_status=None,
                         fastq_offset=33, lower_n_is_base=False):
        """k_pack_text on buffers resident in HBM (DeviceBuffer or raw pointers): the text (capacity round_up(text_bytes, 16)) and
        the uploaded descriptors of text_rows() -> the packed matrix, the lengths, the has-N flags; d_status is a device
        int64[2] the caller set to INT64_MAX.  Asynchronous on the engine's stream."""
        ptr = lambda b: (b.ptr if isinstance(b, DeviceBuffer) else b)
        L.check(self.lib.mpb_pack_text_device(self.ctx, ptr(d_text), int(text_bytes), ptr(d_rows), int(n), int(fastq_offset),
                                              1 if lower_n_is_base else 0, int(stride), ptr(d_q_out), ptr(d_len_out),
                                              ptr(d_flags_out) if d_flags_out is not None else None, ptr(d_status)))

    def filter_text(self, buf, idx, sel=None, fastq_offset=33, max_len=0, lower_n_is_base=False, poisson=False, out=None, **kw):
        """A chunk of FASTQ text in host memory + its record index (fastio.index, or the contigs' buffer and index) ->
        TextFilterResult: the text is uploaded once, packed on the device and filtered there (mpb_filter_text_host); results
        are those of fastio.pack + filter() / filter_poisson() on the same records, bit for bit.  `kw` as filter()'s.
        ValueError with the library's message for a quality character out of range or an index the text cannot hold
        (.bad_record = the record's position in sel order); `out` = (ee, ns, pass, lens, flags) arrays to fill."""
        params = kw.pop("params", None) or self.params(**kw)
        idx, sel, n = _index_args(idx, sel)
        keep, addr, nbytes = _text_ptr(buf)
        r = _TextResults(n, out)
        counts, bad = L.FilterCounts(), C.c_int64(-1)
        rc = self.lib.mpb_filter_text_host(self.ctx, addr, nbytes, idx.ctypes.data, len(idx),
                                           sel.ctypes.data if sel is not None else None, n, int(fastq_offset), int(max_len),
                                           1 if lower_n_is_base else 0, C.byref(params), 1 if poisson else 0, *r.ptrs(),
                                           C.byref(counts), C.byref(bad))
        del keep
        _check_text(rc, bad)
        return TextFilterResult(*r.cut(n), counts.n_pass, counts.n_overflow)

    # ---- the FASTQ record index on the device (k_fq_lines / _scan / _starts / _rows) --------------
    def _fastq_call(self, buf, final, max_records, max_len, call):
        """Either text-alone entry: call(addr, nbytes, final, max_records, max_len, idx, cap, n, consumed, bad, why) -> rc.
        max_records None: no limit; the index is sized by a guess of the records (64 bytes each) and, where the text holds
        more, once more by what the entry counted (_ask_again).  -> (rc, idx rows, n, consumed, bad kind, why)."""
        keep, addr, nbytes = _text_ptr(buf)
        limit = _record_limit(max_records)
        last = None

        def one(cap, _):
            nonlocal last
            idx = np.empty((cap, 6), np.int64)
            n, consumed, bad, why = C.c_int64(0), C.c_int64(0), C.c_int32(0), C.c_int32(0)
            rc = call(addr, nbytes, 1 if final else 0, limit, int(max_len), idx.ctypes.data, cap, C.byref(n), C.byref(consumed),
                      C.byref(bad), C.byref(why))
            last = idx, n.value, consumed.value, bad.value, why.value
            return rc, n.value + 1, None
        rc, _ = _ask_again(one, min(limit, nbytes // 64 + 64) + 1, limit)
        del keep
        return (rc,) + last

    def fastq_index(self, buf, final=True, max_records=None):
        """The record index of a chunk of FASTQ text in host memory, built on the device from the text alone
        (mpb_fastq_index_host) -> (idx int64[n, 6], consumed, bad) as fastio.index returns them: bad is None or a
        fastio.RecordError (.kind, .header, and .row = the six columns of the offending record).  NotTaken(why) when the device
        hands the text back (a lone carriage return, a byte >= 0x80, ...): the caller indexes it on the host."""
        call = lambda *a: self.lib.mpb_fastq_index_host(self.ctx, *a)
        rc, idx, n, consumed, bad, why = self._fastq_call(buf, final, max_records, 0, call)
        L.check(rc)
        if why:
            raise NotTaken(why)
        return idx[:n], consumed, _record_error(buf, idx, n, bad)

    def filter_fastq(self, buf, final=True, max_records=None, fastq_offset=33, max_len=0, lower_n_is_base=False, poisson=False, **kw):
        """A chunk of FASTQ text ALONE -> FastqFilterResult: one upload, the index built on the device, the records before the
        first bad one packed and filtered there (mpb_filter_fastq_host).  .idx, .consumed, .bad are fastio.index's and the
        results are filter_text's on that index, bit for bit.  NotTaken(why) when the device hands the text back; ValueError
        with the library's message for a quality character out of range (.bad_record = the record's position).  `kw` as
        filter()'s."""
        params = kw.pop("params", None) or self.params(**kw)
        counts, badrec = L.FilterCounts(), C.c_int64(-1)
        r = None

        def call(addr, nbytes, final_, limit, max_len_, idx_ptr, cap, n, consumed, bad, why):
            nonlocal r
            r = _TextResults(cap)
            return self.lib.mpb_filter_fastq_host(self.ctx, addr, nbytes, final_, limit, max_len_, idx_ptr, cap, n, consumed, bad, why,
                                                  int(fastq_offset), 1 if lower_n_is_base else 0, C.byref(params), 1 if poisson else 0,
                                                  *r.ptrs(), C.byref(counts), C.byref(badrec))
        rc, idx, n, consumed, bad, why = self._fastq_call(buf, final, max_records, max_len, call)
        _check_text(rc, badrec)
        if why:
            raise NotTaken(why)
        res = FastqFilterResult(idx[:n], consumed, _record_error(buf, idx, n, bad), *r.cut(n), counts.n_pass, counts.n_overflow)
        res.resident = self.resident_text()
        return res

    # ---- fasta+qual input on the device (the index's line kernels, k_fa_count / _scan / _write) ----
    def _fasta_qual_call(self, fbuf, qbuf, final, max_records, max_len, call):
        """Either fasta+qual entry: call(the entry's arguments up to bad_record) -> rc.  out is sized 2 * len(fbuf) + 16, an upper
        bound on the slots, so it never fills; the index by a guess of the records and, where the texts hold more, once more by
        what the entry counted (_ask_again).  -> (rc, out, idx rows, n, f_consumed, q_consumed, out_used, why, which, bad_record)."""
        fkeep, faddr, fbytes = _text_ptr(fbuf)
        qkeep, qaddr, qbytes = _text_ptr(qbuf)
        limit = _record_limit(max_records)
        out = np.empty(2 * fbytes + 16, np.uint8)
        last = None

        def one(cap, _):
            nonlocal last
            idx = np.empty((cap, 6), np.int64)
            n, fc, qc, used, bad = (C.c_int64(0) for _ in range(5))
            why, which = C.c_int32(0), C.c_int32(0)
            rc = call(faddr, fbytes, qaddr, qbytes, 1 if final else 0, limit, int(max_len), out.ctypes.data, len(out), idx.ctypes.data, cap,
                      C.byref(n), C.byref(fc), C.byref(qc), C.byref(used), C.byref(why), C.byref(which), C.byref(bad))
            last = out, idx, n.value, fc.value, qc.value, used.value, why.value, which.value, bad.value
            return rc, n.value, None
        rc, _ = _ask_again(one, min(limit, fbytes // 64 + 64), limit)
        del fkeep, qkeep
        return (rc,) + last

    @staticmethod
    def _fasta_qual_not_taken(why, which, bad):
        return NotTaken(why, which, bad if bad >= 0 else None)

    def fasta_qual_index(self, fbuf, qbuf, final=True, max_records=None):
        """A chunk of fasta text and a chunk of qual text in host memory -> (out, idx, f_consumed, q_consumed): the slots
        header | sequence | one byte per quality (a uint8 array) and their record index, built on the device from the texts
        alone (mpb_fasta_qual_index_host), as fastio.fasta_qual_index builds them.  NotTaken(why, which) when the device hands
        the texts back (.bad_record: the first offending record where there is one): the caller goes through the host function."""
        call = lambda *a: self.lib.mpb_fasta_qual_index_host(self.ctx, *a)
        rc, out, idx, n, fc, qc, used, why, which, bad = self._fasta_qual_call(fbuf, qbuf, final, max_records, 0, call)
        L.check(rc)
        if why:
            raise self._fasta_qual_not_taken(why, which, bad)
        return out[:used], idx[:n], fc, qc

    def filter_fasta_qual(self, fbuf, qbuf, final=True, max_records=None, max_len=0, lower_n_is_base=False, poisson=False, **kw):
        """A chunk of fasta text and a chunk of qual text ALONE -> FastaQualFilterResult: one upload, slots and index built on
        the device, the records packed and filtered there (mpb_filter_fasta_qual_host).  .text, .idx, .f_consumed, .q_consumed
        are fastio.fasta_qual_index's and the results are filter_text's (fastq_offset=0) on them, bit for bit.  NotTaken(why,
        which) when the device hands the texts back.  `kw` as filter()'s."""
        params = kw.pop("params", None) or self.params(**kw)
        counts, badrec = L.FilterCounts(), C.c_int64(-1)
        r = None

        def call(*a):
            nonlocal r
            r = _TextResults(max(a[10], 1))                  # (a[10]: the rows of this try)
            return self.lib.mpb_filter_fasta_qual_host(self.ctx, *a, 1 if lower_n_is_base else 0, C.byref(params), 1 if poisson else 0,
                                                       *r.ptrs(), C.byref(counts), C.byref(badrec))
        rc, out, idx, n, fc, qc, used, why, which, bad = self._fasta_qual_call(fbuf, qbuf, final, max_records, max_len, call)
        _check_text(rc, badrec)
        if why:
            raise self._fasta_qual_not_taken(why, which, bad)
        res = FastaQualFilterResult(out[:used], idx[:n], fc, qc, *r.cut(n), counts.n_pass, counts.n_overflow)
        res.resident = self.resident_text()
        return res

    # ---- BGZF FASTQ filtered where it inflates (k_bgzf_inflate, k_bgzf_crc32, the index, the pack) ----
    def crc32_ranges(self, buf, offs, lens):
        """The CRC-32 (zlib.crc32's) of buf[offs[k] : offs[k] + lens[k]] for every k, computed on the device (mpb_crc32_ranges_host:
        one upload, k_bgzf_crc32, one read-back) -> a uint32 array.  A range holds 0 .. 65536 bytes at any offset; ranges may
        overlap.  ValueError for a range outside the text.  The kernel is timed under kernel_times()["bgzf_inflate"]."""
        keep, addr, nbytes = _text_ptr(buf)
        offs = np.ascontiguousarray(offs, np.int64)
        lens = np.ascontiguousarray(lens, np.int32)
        if offs.ndim != 1 or offs.shape != lens.shape:
            raise ValueError("crc32_ranges: offs and lens must be one-dimensional and equally long")
        out = np.zeros(len(offs), np.uint32)
        L.check(self.lib.mpb_crc32_ranges_host(self.ctx, addr, nbytes, offs.ctypes.data, lens.ctypes.data, len(offs), out.ctypes.data))
        del keep
        return out

    def filter_bgzf_fastq(self, data, offs, sizes, out_offs, carry=b"", final=True, max_records=None, fastq_offset=33, max_len=0,
                          lower_n_is_base=False, poisson=False, text=True, **kw):
        """The BGZF members of `data` (bgzf_inflate's arguments) holding FASTQ text, behind `carry` (the partial record the call
        before left) -> BgzfFastqFilterResult: compressed bytes go up, the members are inflated into the buffer the device
        indexes, their CRC-32 is checked there, and the records are packed and filtered where they lie
        (mpb_filter_bgzf_fastq_host).  Results are filter_fastq's on carry + the inflated text, bit for bit; .idx, .consumed and
        .bad are relative to that text, which comes back as .text unless text=False (.bad then has no header); text may also be
        a uint8 array to write it into (.text is then a view of it).
        MembersNotTaken when a member is handed back (nothing was filtered); NotTaken(why) when the index hands the text back;
        ValueError for a quality character out of range (.bad_record).  `kw` as filter()'s."""
        params = kw.pop("params", None) or self.params(**kw)
        src = data if isinstance(data, np.ndarray) else np.frombuffer(memoryview(data).cast("B"), np.uint8)
        offs = np.ascontiguousarray(offs, np.int64)
        sizes = np.ascontiguousarray(sizes, np.int32)
        out_offs = np.ascontiguousarray(out_offs, np.int64)
        m = len(offs)
        if src.dtype != np.uint8 or not src.flags.c_contiguous or len(sizes) != m or len(out_offs) != m + 1:
            raise ValueError("filter_bgzf_fastq: data must be contiguous bytes, sizes as long as offs, out_offs one longer")
        ckeep, caddr, clen = _text_ptr(carry)
        total = clen + int(out_offs[m])
        if isinstance(text, np.ndarray):                     # the caller's own buffer (one that earlier calls have touched is
            tbuf = text                                       # filled several times faster than fresh pages are)
            if tbuf.dtype != np.uint8 or not tbuf.flags.c_contiguous or tbuf.ndim != 1 or len(tbuf) < total:
                raise ValueError("filter_bgzf_fastq: text must be a contiguous uint8 array of at least %d bytes" % total)
            text = True
        else:
            tbuf = np.empty(max(total, 1), np.uint8) if text else None
        done, mwhy, st = np.zeros(max(m, 1), np.uint8), np.zeros(max(m, 1), np.uint8), L.BgzfInflateStats()
        first = C.c_int64(-1)
        counts, badrec = L.FilterCounts(), C.c_int64(-1)
        limit = _record_limit(max_records)
        idx = r = n = consumed = bad = why = None

        def call(cap, _):
            nonlocal idx, r, n, consumed, bad, why
            idx, r = np.empty((cap, 6), np.int64), _TextResults(cap)
            n, consumed, bad, why = C.c_int64(0), C.c_int64(0), C.c_int32(0), C.c_int32(0)
            rc = self.lib.mpb_filter_bgzf_fastq_host(
                self.ctx, caddr if clen else None, clen, src.ctypes.data, len(src), offs.ctypes.data, sizes.ctypes.data,
                out_offs.ctypes.data, m, 1 if final else 0, limit, int(max_len), tbuf.ctypes.data if text else None,
                len(tbuf) if text else 0, done.ctypes.data, mwhy.ctypes.data, C.byref(first), C.byref(st), idx.ctypes.data, cap,
                C.byref(n), C.byref(consumed), C.byref(bad), C.byref(why), int(fastq_offset), 1 if lower_n_is_base else 0,
                C.byref(params), 1 if poisson else 0, *r.ptrs(), C.byref(counts), C.byref(badrec))
            return rc, (n.value + 1 if first.value < 0 else 0), None      # (no more rows to ask for once a member was handed back)
        rc, _ = _ask_again(call, min(limit, total // 64 + 64) + 1, limit)   # (_fastq_call's guess; the whole call once more)
        del ckeep
        _check_text(rc, badrec)
        stats = {k: int(getattr(st, k)) for k, _ in L.BgzfInflateStats._fields_}
        if first.value >= 0:
            raise MembersNotTaken(first.value, done[:m], mwhy[:m])
        if why.value:
            raise NotTaken(why.value)
        n = n.value
        tout = tbuf[:total] if text else None
        res = BgzfFastqFilterResult(tout, stats, idx[:n], consumed.value, _record_error(tout, idx, n, bad.value), *r.cut(n),
                                    counts.n_pass, counts.n_overflow)
        res.resident = self.resident_text()
        return res

    # ---- output records formatted on the device (k_fmt_count, k_fmt_scan, k_fmt_write) -------------
    def resident_text(self):
        """The generation of the text and index the last filter_fastq / filter_bgzf_fastq / filter_fasta_qual call left on the device;
        0: none."""
        return int(self.lib.mpb_resident_text(self.ctx))

    def format_text(self, buf=None, idx=None, sel=None, kind=2, resident=None, bgzf=False, fastq_offset=33, max_len=0, relabel=None,
                    relabel_index=None, labels=None, label_id=None, out_offset=None, clamp_q0=True, ee=None, records_entry=False):
        """Records sel (None: all) of a text and its record index as fasta (kind 0), qual (1) or fastq (2) text, formatted on
        the device (mpb_format_text_host; with ee, one float64 per selected record: mpb_format_records_host, which puts
        ";ee=%.2f;size=1;" behind the header token): byte for byte fastio.format_records' on the same arguments.  An ee that is
        not finite or not below 2^53 is a ValueError with .bad_record = k: the caller formats on the host.
        records_entry=True: through mpb_format_records_host without ee as well (the same bytes; mpb_format_text_host is that call).
        buf + idx: the text and index go up once.  resident=g (a filter result's .resident; buf None): the text and index that
        call left on the device are read where they lie; idx is then the result's .idx, used for the record count and to size
        the output only.  -> bytes; with bgzf=True a uint8 array of the BGZF members of that text, compressed where it lies,
        without the end marker -- the bytes bgzf_compress returns for it (the counts: bgzf_stats()).
        NotResident for a generation that is no longer in force; ValueError with .bad_record = k for a selected record whose
        row, sel, relabel_index or label_id entry fails a check (nothing is written then)."""
        return self._format_records("format_text", buf, idx, sel, kind, resident, bgzf, fastq_offset, max_len, relabel, relabel_index,
                                    labels, label_id, out_offset, clamp_q0, ee, None, records_entry)

    def format_report(self, buf=None, idx=None, aux=None, sel=None, resident=None, bgzf=False, relabel=None, relabel_index=None, ee=None):
        """The contigs.report lines of records sel (None: all), formatted on the device (mpb_format_records_host, kind 4): byte
        for byte fastio.format_report's on the same arguments.  buf + idx + aux (int32[n_records, 3], by record): all go up.
        resident=g (a contigs_filter_fastq result's .resident; buf and aux None): the slots, their index and the device's own
        overlap / gaps / mismatches arrays are read where they lie; idx is then the result's .cidx.  -> bytes, or BGZF members as
        format_text.  NotResident for a generation that is no longer in force; ValueError for a generation that carries no aux
        (a single-end text), and with .bad_record = k for a selected record that fails a check or an ee outside the domain."""
        if not resident:
            if aux is None:
                raise ValueError("format_report: aux is needed with buf and idx")
            aux = np.ascontiguousarray(aux, np.int32)
            if idx is not None and aux.shape != (len(idx), 3):
                raise ValueError("format_report: aux must be int32[n_records, 3]")
        elif aux is not None:
            raise ValueError("format_report: either buf, idx and aux or resident, not both")
        return self._format_records("format_report", buf, idx, sel, 4, resident, bgzf, 33, 0, relabel, relabel_index, None, None, None,
                                    True, ee, aux)

    def _format_records(self, who, buf, idx, sel, kind, resident, bgzf, fastq_offset, max_len, relabel, relabel_index, labels, label_id,
                        out_offset, clamp_q0, ee, aux, records_entry=False):
        if idx is None:
            raise ValueError("%s: idx is needed (resident form: the result's index)" % who)
        idx, sel, nsel = _index_args(idx, sel)
        if resident is None or not resident:
            if buf is None:
                raise ValueError("%s: either buf and idx or resident" % who)
            keep, addr, nbytes = _text_ptr(buf)
            gen = 0
        else:
            if buf is not None:
                raise ValueError("%s: either buf and idx or resident, not both" % who)
            keep, addr, nbytes, gen = None, None, 0, int(resident)
        if relabel is not None:
            relabel = relabel.encode() if isinstance(relabel, str) else bytes(relabel)
            if relabel_index is None:
                raise ValueError("%s: relabel without relabel_index" % who)
            relabel_index = np.ascontiguousarray(relabel_index, np.int64).reshape(-1)
            if len(relabel_index) != nsel:
                raise ValueError("%s: relabel_index must hold one entry per selected record" % who)
        enc, lab_arr = [], None
        if label_id is not None:
            label_id = np.ascontiguousarray(label_id, np.int32).reshape(-1)
            if len(label_id) != nsel:
                raise ValueError("%s: label_id must hold one entry per selected record" % who)
            enc = [t.encode() if isinstance(t, str) else bytes(t) for t in (labels or [])]
            lab_arr = (C.c_char_p * max(len(enc), 1))(*enc)
        # an upper bound of the formatted text from the index: the call never has to be made twice
        n = len(idx)
        rows = idx if sel is None else idx[sel[(sel >= 0) & (sel < n)]]
        lens = np.clip(rows[:, 3], 0, 1 << 31)
        if max_len > 0:
            lens = np.minimum(lens, int(max_len))
        body = {0: lens + 1, 1: 4 * lens + 1, 2: 2 * lens + 4, 4: 0 * lens + 40}.get(int(kind), lens)
        head = (len(relabel) + 20) if relabel is not None else np.clip(rows[:, 1], 0, 1 << 31)
        bound = int(np.sum(body + head)) + nsel * (3 + max([len(t) for t in enc] + [0]))
        if ee is not None:
            ee = np.ascontiguousarray(ee, np.float64).reshape(-1)
            if len(ee) != nsel:
                raise ValueError("%s: ee must hold one entry per selected record" % who)
            bound += 32 * nsel
        cap = C.c_int64(bound)
        if bgzf:
            L.check(self.lib.mpb_bgzf_bound(bound, C.byref(cap)))
        out = np.empty(max(cap.value, 1), np.uint8)
        got, needed, bad, st = C.c_int64(0), C.c_int64(0), C.c_int64(-1), L.BgzfStats()
        off = int(fastq_offset)
        head_args = (self.ctx, addr, nbytes, idx.ctypes.data if not gen else None, n, gen, sel.ctypes.data if sel is not None else None,
                     nsel, int(kind), off, off if out_offset is None else int(out_offset), 1 if clamp_q0 else 0, int(max_len), relabel,
                     relabel_index.ctypes.data if relabel is not None else None,
                     C.cast(lab_arr, C.c_void_p) if lab_arr is not None else None, len(enc),
                     label_id.ctypes.data if label_id is not None else None)
        tail_args = (1 if bgzf else 0, out.ctypes.data, cap.value, C.byref(got), C.byref(needed), C.byref(bad), C.byref(st))
        if ee is None and aux is None and int(kind) != 4 and not records_entry:
            rc = self.lib.mpb_format_text_host(*(head_args + tail_args))
        else:
            rc = self.lib.mpb_format_records_host(*(head_args + (ee.ctypes.data if ee is not None else None,
                                                                 aux.ctypes.data if aux is not None else None) + tail_args))
        del keep
        if rc == L.E_INVALID and b"is not resident" in self.lib.mpb_last_error():
            raise NotResident(self.lib.mpb_last_error().decode(errors="replace"))
        _check_text(rc, bad)
        if bgzf:
            self._bgzf_stats = {k: int(getattr(st, k)) for k, _ in L.BgzfStats._fields_}
            return out[:got.value]
        return out[:got.value].tobytes()

    # ---- the data-parallel part of collapse on the device (k_col_hash, k_col_group, k_col_rep) -----
    def collapse_text(self, buf=None, idx=None, resident=None, n=None, max_len=0):
        """For every record of a text and its record index: the CPython-2.7 hash of its (truncated) sequence and the first record
        of the chunk with the same sequence (mpb_collapse_text_host) -> (hash uint64[n], rep int32[n]), what
        fastio.Collapse.add(hash=, rep=) takes.  buf + idx: both go up once.  resident=g (a filter result's .resident; buf
        None): the text and index that call left on the device are read where they lie; the record count is n, or len(idx)
        of the result's .idx.  The generation stays in force.  NotResident for a generation that no longer is; ValueError
        with .bad_record = k for a record whose sequence range does not lie inside the text."""
        if resident is None or not resident:
            if buf is None or idx is None:
                raise ValueError("collapse_text: either buf and idx or resident")
            idx = np.ascontiguousarray(idx, np.int64)
            if idx.ndim != 2 or idx.shape[1] != 6:
                raise ValueError("collapse_text: idx must be an (n x 6) int64 record index")
            keep, addr, nbytes, gen, count = *_text_ptr(buf), 0, len(idx)
        else:
            if buf is not None:
                raise ValueError("collapse_text: either buf and idx or resident, not both")
            if n is None and idx is None:
                raise ValueError("collapse_text: the resident form needs n (or the filter result's .idx)")
            keep, addr, nbytes, gen, count = None, None, 0, int(resident), int(len(idx) if n is None else n)
        hash_, rep, bad = np.empty(count, np.uint64), np.empty(count, np.int32), C.c_int64(-1)
        rc = self.lib.mpb_collapse_text_host(self.ctx, addr, nbytes, idx.ctypes.data if not gen else None, count, gen, int(max_len),
                                             hash_.ctypes.data, rep.ctypes.data, C.byref(bad))
        del keep
        if rc == L.E_INVALID and b"is not resident" in self.lib.mpb_last_error():
            raise NotResident(self.lib.mpb_last_error().decode(errors="replace"))
        _check_text(rc, bad)
        return hash_, rep

    # ---- paired-read contigs on the device (mpb_pair_rows, k_contig) ------------------------------
    @staticmethod
    def pair_rows(fidx, ridx, ftext_bytes, rtext_bytes, rec_cap):
        """The validated pair descriptors of k_contig: see the module's pair_rows (host only, needs no device)."""
        return pair_rows(fidx, ridx, ftext_bytes, rtext_bytes, rec_cap)

    def contigs_text(self, fbuf, fidx, rbuf, ridx, fastq_offset=33, match=1, mismatch=-1, gap=-2, insert=20, deltaq=6,
                     consensus=0, qscore_cap=40, trim_overlap=False, rec_cap=None, alignments=False, filter=None):
        """Contigs of a chunk of paired records that are still FASTQ text, built on the device (mpb_contigs_text_host; consensus
        0 best, 1 sum, 2 posterior) -> ContigResult: cbuf / cidx / aux as moira_amd.contig.contigs_from_fastq returns them and
        done (bool per pair).  Slot, index row and aux row of a pair with done == False are undefined: the device handed it
        back and the host aligner builds it (contigs_from_fastq(..., engine=...) does).  alignments=True also returns the
        aligned strings and scores (aln uint8[n, 2, aln_cap], aln_len, score).
        filter: what contigs_filter_text hands on (the one marshalling of a chunk serves both entries); not for callers."""
        fidx, ridx = np.ascontiguousarray(fidx, np.int64), np.ascontiguousarray(ridx, np.int64)
        if fidx.ndim != 2 or fidx.shape[1] != 6 or fidx.shape != ridx.shape:
            raise ValueError("fidx and ridx must be (n x 6) int64 record indexes of the same length")
        n = len(fidx)
        fkeep, faddr, fbytes = _text_ptr(fbuf)
        rkeep, raddr, rbytes = _text_ptr(rbuf)
        if rec_cap is None:
            rec_cap = int((fidx[:, 1] + 2 * (fidx[:, 3] + ridx[:, 3])).max()) + 8 if n else 8
        cbuf, cidx = np.empty(n * rec_cap, np.uint8), np.empty((n, 6), np.int64)
        aux = np.empty((3, n), np.int32)
        done = np.zeros(n, np.uint8)
        aln = aln_len = score = None
        aln_cap = 0
        if alignments:
            aln_cap = max(int((fidx[:, 3] + ridx[:, 3]).max()) if n else 1, 1)
            aln, aln_len, score = np.zeros((n, 2, aln_cap), np.uint8), np.zeros(n, np.int32), np.zeros(n, np.int32)
        prm = _contig_params(match, mismatch, gap, insert, deltaq, consensus, qscore_cap, trim_overlap)
        n_done, n_back, bad = C.c_int64(0), C.c_int64(0), C.c_int64(-1)
        chunk = (self.ctx, faddr, fbytes, fidx.ctypes.data, raddr, rbytes, ridx.ctypes.data, n,
                 int(fastq_offset), C.byref(prm), int(rec_cap), cbuf.ctypes.data, cidx.ctypes.data,
                 aux[0].ctypes.data, aux[1].ctypes.data, aux[2].ctypes.data, done.ctypes.data,
                 aln.ctypes.data if alignments else None, aln_cap,
                 aln_len.ctypes.data if alignments else None, score.ctypes.data if alignments else None,
                 C.byref(n_done), C.byref(n_back), C.byref(bad))
        if filter is None:
            rc = self.lib.mpb_contigs_text_host(*chunk)
        else:
            max_len, lower_n_is_base, poisson, params, r = filter
            filtered = np.zeros(n, np.uint8)
            counts, frc, fbad = L.FilterCounts(), C.c_int(0), C.c_int64(-1)
            rc = self.lib.mpb_contigs_filter_text_host(*chunk, int(max_len), 1 if lower_n_is_base else 0, C.byref(params),
                                                       1 if poisson else 0, *r.ptrs(), filtered.ctypes.data, C.byref(counts),
                                                       C.byref(frc), C.byref(fbad))
        del fkeep, rkeep
        _check_text(rc, bad)
        res = ContigResult(cbuf, cidx, np.ascontiguousarray(aux.T), done.view(bool), rec_cap, n_done.value, n_back.value, aln, aln_len, score)
        if filter is None:
            return res
        return ContigFilterResult(res, *r.cut(n), filtered.view(bool), counts.n_pass, counts.n_overflow, _filter_error(frc, fbad))

    def contigs_filter_text(self, fbuf, fidx, rbuf, ridx, fastq_offset=33, match=1, mismatch=-1, gap=-2, insert=20, deltaq=6,
                            consensus=0, qscore_cap=40, trim_overlap=False, rec_cap=None, alignments=False, max_len=0,
                            lower_n_is_base=False, poisson=False, out=None, **kw):
        """contigs_text and filter_text in one call that keeps the chunk on the device (mpb_contigs_filter_text_host): the contigs
        are built, then packed and filtered in the slots they were written to, and everything comes back at the end ->
        ContigFilterResult.  For the pairs with filtered == True (the pairs the device built, unless the chunk's filter was
        refused) ee / ns / passed / lens / has_n are those of filter_text(cbuf, cidx, sel=those pairs), bit for bit; for the
        others they are undefined and the caller filters them once the host has built them (moira_amd.contig.
        contigs_from_fastq_filtered does).  max_len, lower_n_is_base, poisson, out and `kw` as filter_text's.  What filter_text
        would have raised for the chunk is returned as filter_error (with .bad_record), not raised: the contigs are valid."""
        params = kw.pop("params", None) or self.params(**kw)
        return self.contigs_text(fbuf, fidx, rbuf, ridx, fastq_offset, match, mismatch, gap, insert, deltaq, consensus, qscore_cap,
                                 trim_overlap, rec_cap=rec_cap, alignments=alignments,
                                 filter=(max_len, lower_n_is_base, poisson, params, _TextResults(len(fidx), out)))

    def contigs_filter_fastq(self, fbuf, rbuf, ffinal=True, rfinal=True, max_records=None, fastq_offset=33, match=1, mismatch=-1,
                             gap=-2, insert=20, deltaq=6, consensus=0, qscore_cap=40, trim_overlap=False, max_len=0,
                             lower_n_is_base=False, poisson=False, idx_cap_rows=None, out_cap_bytes=None, **kw):
        """contigs_filter_text from the two mates' FASTQ text ALONE (mpb_contigs_filter_fastq_host): both record indexes, the header
        comparison, the pair descriptors and the class lists are made on the device -> PairedFastqResult.  .fidx, .ridx, .f_bad,
        .r_bad, .f_consumed, .r_consumed and .mismatch are the host indexer's, and every other field is contigs_filter_text's on
        those two indexes cut to .n_built pairs, bit for bit.  NotTaken(why) with .which (0 forward, 1 reverse) when the device
        hands a text back.  idx_cap_rows / out_cap_bytes: the first guess of the two capacities (None: from the texts' sizes);
        where a guess is too small the entry says what is needed and is asked again."""
        params = kw.pop("params", None) or self.params(**kw)
        fkeep, faddr, fbytes = _text_ptr(fbuf)
        rkeep, raddr, rbytes = _text_ptr(rbuf)
        limit = _record_limit(max_records)
        cap = int(idx_cap_rows) if idx_cap_rows is not None else min(limit, max(fbytes, rbytes) // 64 + 64) + 1
        out_cap = int(out_cap_bytes) if out_cap_bytes is not None else 2 * (fbytes + rbytes) + 16 * cap
        prm = _contig_params(match, mismatch, gap, insert, deltaq, consensus, qscore_cap, trim_overlap)
        i64 = lambda v=0: C.c_int64(v)
        fidx = ridx = cbuf = cidx = aux = done = r = filtered = n_f = n_r = n_pairs = mis = n_built = f_cons = r_cons = rec_cap = None
        f_kind = r_kind = why = which = n_done = n_back = counts = frc = fbad = None

        def call(cap, out_cap):
            nonlocal fidx, ridx, cbuf, cidx, aux, done, r, filtered, n_f, n_r, n_pairs, mis, n_built, f_cons, r_cons, rec_cap
            nonlocal f_kind, r_kind, why, which, n_done, n_back, counts, frc, fbad
            fidx, ridx = np.empty((cap, 6), np.int64), np.empty((cap, 6), np.int64)
            cbuf, cidx, aux, done = np.empty(out_cap, np.uint8), np.empty((cap, 6), np.int64), np.empty((3, cap), np.int32), np.zeros(cap, np.uint8)
            r, filtered = _TextResults(cap), np.zeros(cap, np.uint8)
            n_f, n_r, n_pairs, mis, n_built, f_cons, r_cons, rec_cap = i64(), i64(), i64(), i64(-1), i64(), i64(), i64(), i64()
            f_kind, r_kind, why, which = C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_int32(0)
            n_done, n_back, counts, frc, fbad = i64(), i64(), L.FilterCounts(), C.c_int(0), i64(-1)
            rc = self.lib.mpb_contigs_filter_fastq_host(
                self.ctx, faddr, fbytes, 1 if ffinal else 0, raddr, rbytes, 1 if rfinal else 0, limit, int(fastq_offset), C.byref(prm),
                fidx.ctypes.data, ridx.ctypes.data, cap, C.byref(n_f), C.byref(f_kind), C.byref(n_r), C.byref(r_kind), C.byref(n_pairs),
                C.byref(mis), C.byref(n_built), C.byref(f_cons), C.byref(r_cons), C.byref(why), C.byref(which), C.byref(rec_cap),
                cbuf.ctypes.data, out_cap, cidx.ctypes.data, aux[0].ctypes.data, aux[1].ctypes.data, aux[2].ctypes.data, done.ctypes.data,
                C.byref(n_done), C.byref(n_back), int(max_len), 1 if lower_n_is_base else 0, C.byref(params), 1 if poisson else 0,
                *r.ptrs(), filtered.ctypes.data, C.byref(counts), C.byref(frc), C.byref(fbad))
            # (bytes: n_built <= n_pairs, so n_pairs slots are enough whatever the headers say; a slot of 8 bytes holds no pair)
            return rc, max(n_f.value, n_r.value) + 1, (n_pairs.value * rec_cap.value if rec_cap.value > 8 else 0)
        rc, calls = _ask_again(call, cap, limit, out_cap, grow_out=out_cap_bytes is None)
        del fkeep, rkeep
        L.check(rc)
        if why.value:
            raise NotTaken(why.value, which.value)
        n = n_built.value
        res = ContigResult(cbuf[:n * rec_cap.value], cidx[:n], np.ascontiguousarray(aux[:, :n].T), done[:n].view(bool), rec_cap.value,
                           n_done.value, n_back.value, None, None, None)
        res = ContigFilterResult(res, *r.cut(n), filtered[:n].view(bool), counts.n_pass, counts.n_overflow, _filter_error(frc, fbad))
        return PairedFastqResult(res, fidx[:n_f.value], ridx[:n_r.value], f_cons.value, r_cons.value,
                                 _record_error(fbuf, fidx, n_f.value, f_kind.value), _record_error(rbuf, ridx, n_r.value, r_kind.value),
                                 mis.value, n_pairs.value, n, calls, self.resident_text())

    def decode_ascii_device(self, d_seq, d_qual, n, stride, d_out, d_len=None, fixed_len=0, fastq_offset=33,
                            d_err=None):
        ptr = lambda b: (b.ptr if isinstance(b, DeviceBuffer) else b)
        L.check(self.lib.mpb_decode_ascii_device(self.ctx, ptr(d_seq), ptr(d_qual), n, stride,
                                                 ptr(d_len) if d_len is not None else None, int(fixed_len),
                                                 int(fastq_offset), ptr(d_out),
                                                 ptr(d_err) if d_err is not None else None))

    def encode_ascii_device(self, d_q, n, stride, d_seq_out, d_qual_out, fastq_offset=33):
        ptr = lambda b: (b.ptr if isinstance(b, DeviceBuffer) else b)
        L.check(self.lib.mpb_encode_ascii_device(self.ctx, ptr(d_q), n, stride, int(fastq_offset), ptr(d_seq_out), ptr(d_qual_out)))

    def filter_ascii_device(self, d_seq, d_qual, n, stride, d_q_out, d_len=None, fixed_len=0, fastq_offset=33,
                            d_ee=None, d_ns=None, d_pass=None, d_err=None, params=None, want_counts=True):
        """Raw FASTQ text resident in HBM -> results, classified at source: the decode pass classifies the reads, the
        filter starts at the scan (mpb_decode_classify_device + mpb_filter_device_classified)."""
        params = params or self.params()
        ptr = lambda b: (b.ptr if isinstance(b, DeviceBuffer) else b)
        opt = lambda b: (ptr(b) if b is not None else None)
        L.check(self.lib.mpb_decode_classify_device(self.ctx, ptr(d_seq), ptr(d_qual), n, stride, opt(d_len), int(fixed_len),
                                                    int(fastq_offset), C.byref(params), ptr(d_q_out), ptr(d_ee), ptr(d_ns),
                                                    ptr(d_pass), opt(d_err)))
        counts = L.FilterCounts()
        L.check(self.lib.mpb_filter_device_classified(self.ctx, ptr(d_q_out), n, stride, opt(d_len), int(fixed_len),
                                                      C.byref(params), ptr(d_ee), ptr(d_ns), ptr(d_pass),
                                                      C.byref(counts) if want_counts else None))
        return counts if want_counts else None

    # ---- the hot path -------------------------------------------------------------------------
    def filter_device(self, d_q, n, stride, d_len=None, fixed_len=0, d_ee=None, d_ns=None, d_pass=None,
                      params=None, want_counts=True):
        """Filter a batch already resident in HBM.  d_* are DeviceBuffer or raw int pointers."""
        params = params or self.params()
        ptr = lambda b: (b.ptr if isinstance(b, DeviceBuffer) else b)
        counts = L.FilterCounts()
        L.check(self.lib.mpb_filter_device(self.ctx, ptr(d_q), n, stride, ptr(d_len) if d_len is not None else None,
                                           int(fixed_len), C.byref(params), ptr(d_ee), ptr(d_ns), ptr(d_pass),
                                           C.byref(counts) if want_counts else None))
        return counts if want_counts else None

    def pack_coded(self, seqs, quals, stride=None, max_len=0):
        """Reads whose scores may exceed 254 (any non-negative int, as moira/bernoullimodule.c:92-108 takes them) ->
        (q uint8[n, stride], lens int32[n], code_scores int32[256]): every distinct score above 254 of the BATCH gets a
        byte code the batch does not use; `code_scores[c]` is what code c stands for.  ValueError (MPB_E_RANGE) when the
        batch has more such scores than free codes.  Pass code_scores on to filter()."""
        n = len(quals)
        off = np.zeros(n + 1, np.int64)
        if n:
            off[1:] = np.cumsum([len(x) for x in quals])
        if seqs is not None and any(len(s) != len(x) for s, x in zip(seqs, quals)):
            raise ValueError("contig and contig_quals must have the same length")
        lens_full = off[1:] - off[:-1]
        longest = int(min(lens_full.max(), max_len) if (n and max_len > 0) else (lens_full.max() if n else 1))
        if stride is None:
            stride = _round_up(max(longest, 1), 16)
        flat = np.concatenate([np.asarray(x, np.int64) for x in quals]) if n and off[-1] else np.empty(0, np.int64)
        if len(flat) and (flat.min() < -(1 << 31) or flat.max() >= (1 << 31)):
            raise ValueError("a quality score does not fit a C int")
        flat = np.ascontiguousarray(flat, np.int32)
        q = np.empty((n, stride), np.uint8)
        lens = np.empty(n, np.int32)
        codes = np.empty(256, np.int32)
        L.check(self.lib.mpb_pack_batch_coded("".join(seqs).encode() if seqs is not None else None, flat.ctypes.data,
                                              off.ctypes.data, n, int(max_len), stride, q.ctypes.data, lens.ctypes.data,
                                              codes.ctypes.data))
        return q, lens, codes

    def filter(self, q, lens=None, fixed_len=None, out=None, code_scores=None, **kw):
        """Filter a packed host matrix q (n x stride uint8).  Returns FilterResult.  code_scores: what pack_coded returned
        (a batch that carries scores above 254)."""
        kw.setdefault("batched_only", self.batched_only)
        params = kw.pop("params", None) or self.params(**kw)
        q, n, stride, lens, (ee, ns, ps) = check_host_batch(q, lens, fixed_len, out, limit=L.MAX_LEN)
        counts = L.FilterCounts()
        if code_scores is not None:
            code_scores = np.ascontiguousarray(code_scores, np.int32)
            if code_scores.shape != (256,):
                raise ValueError("code_scores must hold 256 entries")
        L.check(self.lib.mpb_filter_host_coded(self.ctx, q.ctypes.data, n, stride,
                                               lens.ctypes.data if lens is not None else None,
                                               0 if lens is not None else int(fixed_len), C.byref(params),
                                               code_scores.ctypes.data if code_scores is not None else None,
                                               ee.ctypes.data, ns.ctypes.data, ps.ctypes.data, C.byref(counts)))
        return FilterResult(ee, ns, ps.view(bool), counts.n_pass, counts.n_overflow)   # pass bytes are 0 / 1

    def filter_poisson(self, q, lens=None, fixed_len=None, out=None, **kw):
        """--error_calc poisson (moira/moira.py:1637-1679): lambda summed on the GPU in base order,
        scalar CDF tail on the host with the reference's libm calls.  Returns FilterResult.
        poisson_device_tail=True (MPB_FLAG_POISSON_DEVICE_TAIL): the tail runs on the GPU too -- ee within 1e-9 relative, ns /
        pass / NaN identical; n_overflow = the reads the host tail finished."""
        params = kw.pop("params", None) or self.params(**kw)
        q, n, stride, lens, (ee, ns, ps) = check_host_batch(q, lens, fixed_len, out, limit=None)
        counts = L.FilterCounts()
        L.check(self.lib.mpb_filter_poisson_host(self.ctx, q.ctypes.data, n, stride,
                                                 lens.ctypes.data if lens is not None else None,
                                                 0 if lens is not None else int(fixed_len), C.byref(params),
                                                 ee.ctypes.data, ns.ctypes.data, ps.ctypes.data, C.byref(counts)))
        return FilterResult(ee, ns, ps.view(bool), counts.n_pass, counts.n_overflow)     # (0 without poisson_device_tail)

    def poisson_finish_device(self, d_lambda, d_ns, n, d_len=None, fixed_len=0, d_ee=None, d_pass=None, params=None,
                              want_counts=True):
        """The device twin of mpb_poisson_finish_host: lambda / ns (/ len) resident in HBM -> ee / pass there.  d_ee may be
        d_lambda.  Synchronises (include/moira_pb.h, "the device tail")."""
        params = params or self.params()
        ptr = lambda b: (b.ptr if isinstance(b, DeviceBuffer) else b)
        counts = L.FilterCounts()
        L.check(self.lib.mpb_poisson_finish_device(self.ctx, ptr(d_lambda), ptr(d_ns), ptr(d_len) if d_len is not None else None,
                                                   int(fixed_len), n, C.byref(params), ptr(d_ee), ptr(d_pass),
                                                   C.byref(counts) if want_counts else None))
        return counts if want_counts else None

    def filter_poisson_device(self, d_q, n, stride, d_len=None, fixed_len=0, d_ee=None, d_ns=None, d_pass=None, d_lambda=None,
                              params=None, want_counts=True):
        """--error_calc poisson on a batch already resident in HBM (k_lambda + the device tail); results stay there.
        d_lambda (optional) receives lambda.  Synchronises."""
        params = params or self.params()
        ptr = lambda b: (b.ptr if isinstance(b, DeviceBuffer) else b)
        counts = L.FilterCounts()
        L.check(self.lib.mpb_filter_poisson_device(self.ctx, ptr(d_q), n, stride, ptr(d_len) if d_len is not None else None,
                                                   int(fixed_len), C.byref(params), ptr(d_ee), ptr(d_ns), ptr(d_pass),
                                                   ptr(d_lambda) if d_lambda is not None else None,
                                                   C.byref(counts) if want_counts else None))
        return counts if want_counts else None

    def calculate_errors_PB(self, contig, contig_quals, alpha):
        """Exact twin of bernoulli.calculate_errors_PB -> (expected_errors, Ns).
        ref: moira/bernoullimodule.c:66-114 (argument and error behaviour)."""
        from .broker import marshal_read               # the argument rules, shared with the broker entry
        seq, qi, addr, alpha = marshal_read(contig, contig_quals, alpha)
        ee, ns = C.c_double(), C.c_int32()
        L.check(self.lib.mpb_calculate_errors_PB(self.ctx, seq, addr, len(qi), alpha,
                                                 C.byref(ee), C.byref(ns)))
        return ee.value, ns.value

    def calculate_errors_poisson(self, sequence, quals, alpha):
        """Twin of moira.py's calculate_errors_poisson(sequence, quals, alpha) -> (expected_errors, Ns)
        (moira/moira.py:1637-1679): lambda summed on the GPU in base order, the scalar tail on the host.  Any
        non-negative int is a score; OverflowError where the Python function raises it."""
        sequence = str(sequence)
        qi = np.array([int(v) for v in quals], np.int64).astype(np.int32) if len(quals) else np.empty(0, np.int32)
        alpha = float(alpha)
        if len(sequence) != len(qi):
            raise ValueError("sequence and quals must have the same length")
        if alpha <= 0 or alpha >= 1:                           # (the bare Python function also takes alpha == 1)
            raise ValueError("Alpha must be between 0 (not included) and 1.")
        ee, ns = C.c_double(), C.c_int32()
        L.check(self.lib.mpb_calculate_errors_poisson(self.ctx, sequence.encode(), qi.ctypes.data, len(qi), alpha,
                                                      C.byref(ee), C.byref(ns)))
        if ee.value != ee.value:
            raise OverflowError("Lambda ** expected_errors or its factorial leaves the float range (moira.py:1671)")
        return ee.value, ns.value

    # ---- synthetic workload -----------------------------------------------------------------------
    def synth_fill(self, d_q, n, stride, fixed_len=0, min_len=0, max_len=0, d_len=None, seed=1, first_read=0, profile=0):
        """profile: 0 = the model of include/mpb_synth.h (BASELINE's configs), 1 = the clean run (Q33..Q40)."""
        ptr = lambda b: (b.ptr if isinstance(b, DeviceBuffer) else b)
        L.check(self.lib.mpb_synth_fill_device_profile(self.ctx, ptr(d_q), n, stride, fixed_len, min_len, max_len,
                                                       ptr(d_len) if d_len is not None else None, seed, first_read, profile))

    def last_path(self):
        """Which pass the last filter_device call took: dict(narrow_rows, narrow_split, narrow_waves, sampled, n_fallback,
        sample_hist)."""
        info = L.PathInfo()
        L.check(self.lib.mpb_last_path(self.ctx, C.byref(info)))
        return {"narrow_rows": info.narrow_rows, "sampled": bool(info.sampled), "n_fallback": info.n_fallback,
                "sample_hist": list(info.sample_hist), "narrow_split": info.narrow_split, "narrow_waves": info.narrow_waves}

    # ---- .gz output on the device -----------------------------------------------------------------
    def bgzf_compress(self, data):
        """`data` (bytes-like) as BGZF members compressed on the device (mpb_bgzf_compress_host: k_bgzf_deflate, k_bgzf_scan,
        k_bgzf_frame), in order, WITHOUT the format's end marker -- the bytes moira_amd.cli.bgzf_compress returns differ (another
        deflate), what they inflate to does not.  The counts of the call: bgzf_stats()."""
        mv = memoryview(data).cast("B")
        n = len(mv)
        src = np.frombuffer(mv, np.uint8) if n else np.empty(0, np.uint8)
        cap = C.c_int64()
        L.check(self.lib.mpb_bgzf_bound(n, C.byref(cap)))
        out = np.empty(max(cap.value, 1), np.uint8)
        got, st = C.c_int64(), L.BgzfStats()
        L.check(self.lib.mpb_bgzf_compress_host(self.ctx, src.ctypes.data if n else None, n, out.ctypes.data, cap.value,
                                                C.byref(got), C.byref(st)))
        self._bgzf_stats = {k: int(getattr(st, k)) for k, _ in L.BgzfStats._fields_}
        return out[:got.value].tobytes()

    def bgzf_stats(self):
        """{members, dynamic, fixed, stored, literals, matches, matched_bytes} of the last bgzf_compress call (None before one)."""
        return getattr(self, "_bgzf_stats", None)

    # ---- BGZF .gz input on the device --------------------------------------------------------------
    def bgzf_inflate(self, data, offs, sizes, out_offs, out=None):
        """The BGZF members of `data` (bytes-like; member k = data[offs[k] : offs[k] + sizes[k]], its text at out_offs[k] ..
        out_offs[k + 1] -- the arrays libmoira_io's mio_bgzf_scan fills) inflated on the device (mpb_bgzf_inflate_host:
        k_bgzf_inflate, one wave per member, then the CRC-32 check on the host).  Returns (text, done, why) as uint8 arrays:
        done[k] = 1 where member k was taken and its CRC and length match, else 0 with why[k] one of MPB_BGZF_WHY_* (names:
        _lib.BGZF_WHY) -- the bytes of such a member in `text` are unspecified and the caller inflates it on the host.  `out`: a
        uint8 array of at least out_offs[-1] bytes to write into.  The counts of the call: bgzf_inflate_stats()."""
        src = data if isinstance(data, np.ndarray) else np.frombuffer(memoryview(data).cast("B"), np.uint8)
        offs = np.ascontiguousarray(offs, np.int64)
        sizes = np.ascontiguousarray(sizes, np.int32)
        out_offs = np.ascontiguousarray(out_offs, np.int64)
        n = len(offs)
        if src.dtype != np.uint8 or not src.flags.c_contiguous or len(sizes) != n or len(out_offs) != n + 1:
            raise ValueError("bgzf_inflate: data must be contiguous bytes, sizes as long as offs, out_offs one longer")
        total = int(out_offs[n])
        if out is None:
            out = np.empty(max(total, 1), np.uint8)
        elif out.dtype != np.uint8 or not out.flags.c_contiguous or len(out) < total:
            raise ValueError("bgzf_inflate: out must be a contiguous uint8 array of at least %d bytes" % total)
        done, why, st = np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.uint8), L.BgzfInflateStats()
        L.check(self.lib.mpb_bgzf_inflate_host(self.ctx, src.ctypes.data, len(src), offs.ctypes.data, sizes.ctypes.data,
                                               out_offs.ctypes.data, n, out.ctypes.data, len(out), done.ctypes.data, why.ctypes.data,
                                               C.byref(st)))
        self._bgzf_inflate_stats = {k: int(getattr(st, k)) for k, _ in L.BgzfInflateStats._fields_}
        return out[:total], done[:n], why[:n]

    def bgzf_inflate_stats(self):
        """{members, taken, handed_back, stored_blocks, fixed_blocks, dynamic_blocks, literals, matches, matched_bytes,
        longest_code} of the last bgzf_inflate call (None before one)."""
        return getattr(self, "_bgzf_inflate_stats", None)

    # ---- measurement ----------------------------------------------------------------------------
    def timing(self, on=True):
        L.check(self.lib.mpb_timing_enable(self.ctx, 1 if on else 0))

    def timing_reset(self):
        L.check(self.lib.mpb_timing_reset(self.ctx))

    def kernel_times(self):
        """{name: (total_ms, launches)} since the last reset (synchronises)."""
        out = {}
        for kid, name in (list(L.KERNEL_NAMES.items()) + list(L.CONTIG_KERNEL_NAMES.items()) + list(L.BGZF_KERNEL_NAMES.items())
                          + list(L.INFLATE_KERNEL_NAMES.items()) + list(L.INDEX_KERNEL_NAMES.items())):
            ms, cnt = C.c_double(), C.c_int64()
            L.check(self.lib.mpb_kernel_time(self.ctx, kid, C.byref(ms), C.byref(cnt)))
            out[name] = (ms.value, cnt.value)
        return out

    def device_lut(self):
        """({1-p}, {p'}) as uploaded to this device (256 doubles each; ref: moira/bernoullimodule.c:202,140-145)."""
        a, b = np.empty(256), np.empty(256)
        L.check(self.lib.mpb_device_lut(self.ctx, a.ctypes.data, b.ctypes.data))
        return a, b

    def algorithmic_cells(self):
        """DP cells the algorithm needs (sum_k min(k + 1, J) per read) for the last filter_device call made with
        params(count_cells=True)."""
        v = C.c_int64()
        L.check(self.lib.mpb_last_algorithmic_cells(self.ctx, C.byref(v)))
        return v.value

    def read_budgets(self, n):
        """Row budget (class cap) of each of the first n reads of the last filter_device call."""
        out = np.empty(n, np.int32)
        L.check(self.lib.mpb_last_read_budgets(self.ctx, out.ctypes.data, n))
        return out

    def class_histogram(self):
        caps = np.zeros(64, np.int32)
        cnts = np.zeros(64, np.int64)
        k = self.lib.mpb_last_class_histogram(self.ctx, caps.ctypes.data, cnts.ctypes.data, 64)
        if k < 0:
            L.check(k)
        return {int(caps[i]): int(cnts[i]) for i in range(k)}


def host_lut():
    """The library's Phred -> ({1-p}, {p'}) table computed on the host (no device needed)."""
    a, b = np.empty(256), np.empty(256)
    L.check(L.load().mpb_host_lut(a.ctypes.data, b.ctypes.data))
    return a, b


_default_engine = None


def default_engine():
    """Process-wide engine on device LOCAL_RANK (or 0)."""
    global _default_engine
    if _default_engine is None:
        import os
        _default_engine = Engine(int(os.environ.get("LOCAL_RANK", "0")))
    return _default_engine
