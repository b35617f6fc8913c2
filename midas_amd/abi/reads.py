"""Alignment records and contig tables as the library takes them, and the BAM / SAM / FASTA readers and the BAM writer."""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

from .core import (ERR_INVALID_ARG, ERR_UNSUPPORTED, MidasSnpsError, P, _Column, addr, cstr, host_call, i32, i64, load_library, ptr,
                   register, vp)


class _Reads(C.Structure):
    _fields_ = [("n_reads", C.c_int64), ("pos", C.c_void_p), ("mapq", C.c_void_p), ("flag", C.c_void_p),
                ("nm", C.c_void_p), ("l_seq", C.c_void_p), ("seq_off", C.c_void_p), ("qual_off", C.c_void_p),
                ("cigar_off", C.c_void_p), ("seq4", C.c_void_p), ("qual", C.c_void_p), ("cigar", C.c_void_p)]


class _Contigs(C.Structure):
    _fields_ = [("n_contigs", C.c_int32), ("n_species", C.c_int32), ("length", C.c_void_p),
                ("species", C.c_void_p), ("read_begin", C.c_void_p), ("ref", C.c_void_p), ("origin", C.c_void_p)]


_counts4 = [P(i64)] * 4      # n_reads, seq_bytes, qual_bytes, n_cigar of a load

register('exported', {
    'midas_bam_open': (i32, [cstr, P(vp), cstr]),
    'midas_bam_close': (None, [vp]),
    'midas_bam_write': (i32, [cstr, i32, P(cstr), vp, P(_Reads), vp, i32, i32, cstr]),
    'midas_bam_n_refs': (i32, [vp]),
    'midas_bam_ref': (i32, [vp, i32, P(cstr), P(i64)]),
    'midas_bam_load': (i32, [vp] + _counts4 + [cstr]),
    'midas_bam_copy': (i32, [vp] + [vp] * 12),
    'midas_bam_columns': (i32, [vp, vp]),
    'midas_bam_open_slice': (i32, [cstr, i32, i32, P(vp), cstr]),
    'midas_bam_slice_facts': (i32, [vp, vp, vp, vp, vp]),
    'midas_bam_slice_marks': (i32, [vp, vp, vp, vp, i64]),
    'midas_bam_open_device': (i32, [cstr, vp, P(vp), cstr]),
    'midas_bam_open_slice_device': (i32, [cstr, i32, i32, vp, P(vp), cstr]),
    'midas_bam_load_device': (i32, [cstr, vp, P(vp)] + _counts4 + [cstr]),
    'midas_bam_payload_on_device': (i32, [vp]),
    'midas_bam_release_file': (None, [vp]),
    'midas_bam_load_resident': (i32, [cstr, vp, P(vp), P(i64), P(i64), cstr]),
    'midas_bam_load_ranges_resident': (i32, [vp, vp, i32, vp, vp, P(i64), P(i64), cstr]),
    'midas_bam_is_resident': (i32, [vp]),
    'midas_bam_open_share_local': (i32, [cstr, i32, i32, P(vp), vp, cstr]),
    'midas_bam_share_locate': (i32, [vp, i32, i64, i64, i64, vp, cstr]),
    'midas_bam_resident_to_columns': (i32, [vp, vp, P(i64), P(i64), P(i64), cstr]),
    'midas_bam_load_ranges_device': (i32, [vp, vp, i32, vp, vp] + _counts4 + [cstr]),
    'midas_bam_load_ranges': (i32, [vp, i32, vp, vp] + _counts4 + [cstr]),
    'midas_bam_open_share': (i32, [cstr, i32, i32, i64, P(vp), vp, cstr]),
    'midas_snps_copy_from_device': (i32, [vp, vp, vp, i64]),
    'midas_snps_inflate_blocks': (i32, [vp, vp, i64, i64, vp, vp, vp, vp, vp, vp, i64, P(i64)]),
    'midas_fasta_load': (i32, [i32, vp, i32, P(vp), cstr]),
    'midas_fasta_n_records': (i64, [vp]),
    'midas_fasta_columns': (i32, [vp, vp, vp]),
    'midas_fasta_close': (None, [vp]),
})
# the SAM decode (run_midas.py snps --sam, genes --sam): listed by themselves (SAM_SYMBOLS)
register('sam', {
    'midas_sam_load_device': (i32, [cstr, vp, P(vp)] + _counts4 + [cstr]),
    'midas_sam_decode_timing': (i32, [vp, vp]),
    'midas_sam_load_device_order': (i32, [cstr, vp, i32, P(vp)] + _counts4 + [cstr]),
    'midas_sam_load_resident': (i32, [cstr, vp, P(vp), P(i64), P(i64), cstr]),
})
SAM_ORDERS = {'coordinate': 0, 'file': 1}        # MIDAS_SAM_ORDER_*
SAM_PHASES = ('map + header', 'upload', 'line index', 'pass 1 (fields)', 'scans', 'pass 2 (payload)', 'sort + gather', 'columns down')

_SOA_DTYPES = {
    'pos': np.int32, 'mapq': np.uint8, 'flag': np.uint16, 'nm': np.int32, 'l_seq': np.int32,
    'seq_off': np.int64, 'qual_off': np.int64, 'cigar_off': np.int64,
    'seq4': np.uint8, 'qual': np.uint8, 'cigar': np.uint32,
}


@dataclass
class ReadsSoA:
    """Alignment records in BAM-native encodings (see midas_snps_reads in the header)."""
    pos: np.ndarray
    mapq: np.ndarray
    flag: np.ndarray
    nm: np.ndarray
    l_seq: np.ndarray
    seq_off: np.ndarray
    qual_off: np.ndarray
    cigar_off: np.ndarray
    seq4: np.ndarray
    qual: np.ndarray
    cigar: np.ndarray
    # (seq4, qual, cigar) as DEVICE addresses + whatever keeps them alive (read_bam(..., payload_on_device=True)): the three
    # arrays above are empty then, and only a Context's batch / pileup -- which copy device to device -- can take the reads
    device: Optional[tuple] = None

    def __post_init__(self):
        for k, dt in _SOA_DTYPES.items():
            setattr(self, k, np.ascontiguousarray(getattr(self, k), dtype=dt))

    @property
    def n_reads(self) -> int:
        return int(self.pos.shape[0])

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k in _SOA_DTYPES}

    @classmethod
    def from_dict(cls, d: dict) -> "ReadsSoA":
        return cls(**{k: d[k] for k in _SOA_DTYPES})

    @classmethod
    def empty(cls) -> "ReadsSoA":
        z = lambda dt, n=0: np.zeros(n, dtype=dt)
        return cls(z(np.int32), z(np.uint8), z(np.uint16), z(np.int32), z(np.int32),
                   z(np.int64, 1), z(np.int64, 1), z(np.int64, 1), z(np.uint8), z(np.uint8), z(np.uint32))

    def _c(self) -> _Reads:
        # (addr: zero-size arrays still have a valid address, and a batch of reads refuses a NULL column -- which an empty
        # payload column beside n_reads > 0, e.g. every l_seq 0, must not turn into)
        payload = (addr(self.seq4), addr(self.qual), addr(self.cigar)) if self.device is None else \
            tuple(C.c_void_p(int(x)) for x in self.device[:3])
        return _Reads(self.n_reads, addr(self.pos), addr(self.mapq), addr(self.flag), addr(self.nm), addr(self.l_seq),
                      addr(self.seq_off), addr(self.qual_off), addr(self.cigar_off), *payload)


class ResidentReads:
    """The records of a BAM decoded on a Context's device with EVERY column left there, in the pileup kernel's own layout
    (read_bam(..., resident=True), midas_bam_load_resident): what the host holds is the count, the bases' total and the native
    handle.  Only that context's Batch takes them -- records [first, first + n) of the handle, where they lie; a host that must
    look into the columns asks Context.fetch_payload, which turns them into an ordinary ReadsSoA (midas_bam_resident_to_columns)."""
    device = ('resident',)        # (read like ReadsSoA.device: "not in host memory")

    def __init__(self, lib, handle, owner, n_reads: int, l_seq_total: int, first: int = 0):
        self._lib, self._h, self.owner = lib, handle, owner
        self._n, self.l_seq_total, self.first = int(n_reads), int(l_seq_total), int(first)

    @property
    def n_reads(self) -> int:
        return self._n

    def to_columns(self, ctx) -> "ReadsSoA":
        """The same records as a ReadsSoA whose SEQ / QUAL / CIGAR are device columns (as read_bam(payload_on_device=True)'s)."""
        sb, qb, nc = C.c_int64(), C.c_int64(), C.c_int64()
        host_call(self._lib.midas_bam_resident_to_columns, self._h, ctx._h, C.byref(sb), C.byref(qb), C.byref(nc))
        _, reads = _bam_columns(self._lib, self._h, self._n, int(sb.value), int(qb.value), int(nc.value), self.owner, on_device=True)
        return reads


@dataclass
class ContigTable:
    """Flattened `contigs` dict of midas/run/snps.py:55-67 (see midas_snps_contigs)."""
    length: np.ndarray        # [n_contigs] int64
    species: np.ndarray       # [n_contigs] int32 index into species ids
    read_begin: np.ndarray    # [n_contigs+1] int64
    ref: np.ndarray           # [sum(length)] uint8
    n_species: int
    ids: list = field(default_factory=list)           # contig ids, table order
    species_ids: list = field(default_factory=list)   # species ids, index order
    origin: Optional[np.ndarray] = None               # [n_contigs] int64 or None: the entries are pieces of longer contigs

    def __post_init__(self):
        if self.origin is not None:
            self.origin = np.ascontiguousarray(self.origin, dtype=np.int64)
        self.length = np.ascontiguousarray(self.length, dtype=np.int64)
        self.species = np.ascontiguousarray(self.species, dtype=np.int32)
        self.read_begin = np.ascontiguousarray(self.read_begin, dtype=np.int64)
        self.ref = np.ascontiguousarray(self.ref, dtype=np.uint8)

    @property
    def n_contigs(self) -> int:
        return int(self.length.shape[0])

    @property
    def n_sites(self) -> int:
        return int(self.length.sum())

    def site_offsets(self) -> np.ndarray:
        out = np.zeros(self.n_contigs + 1, dtype=np.int64)
        np.cumsum(self.length, out=out[1:])
        return out

    def _c(self) -> _Contigs:
        # (addr: as ReadsSoA._c; a NULL origin says the entries are whole contigs)
        return _Contigs(self.n_contigs, int(self.n_species), addr(self.length), addr(self.species), addr(self.read_begin),
                        addr(self.ref), addr(self.origin))


def _inflates(ctx) -> bool:
    return ctx is not None and getattr(ctx, 'inflates', False)


def _i64s(n):
    """n int64 outputs and their references, in order."""
    vals = [C.c_int64() for _ in range(n)]
    return vals, [C.byref(v) for v in vals]


def _bam_refs(lib, h):
    names, lens = [], []
    for i in range(lib.midas_bam_n_refs(h)):
        nm = C.c_char_p()
        ln = C.c_int64()
        lib.midas_bam_ref(h, i, C.byref(nm), C.byref(ln))
        names.append(nm.value.decode())
        lens.append(int(ln.value))
    return names, lens


class _BamOwner:
    """Keeps a decoded BAM alive for as long as a numpy view of one of its columns is (midas_bam_columns: no copies)."""

    def __init__(self, lib, h):
        self._lib, self._h = lib, h

    def __del__(self):
        if self._h:
            self._lib.midas_bam_close(self._h)
            self._h = None


def _bam_columns(lib, h, n, sb, qb, nc, owner=None, on_device=False):
    """(refid, ReadsSoA) over the decoder's own buffers.  `owner` (a _BamOwner) is kept alive by every array.  on_device:
    the last three columns are device addresses (midas_bam_load_device) and go into ReadsSoA.device."""
    ptrs = (C.c_void_p * 12)()
    st = lib.midas_bam_columns(h, ptrs)
    if st != 0:
        raise MidasSnpsError(st, "midas_bam_columns failed")
    if owner is None:
        owner = _BamOwner(lib, None)      # (the caller keeps the handle itself)
    spec = [('refid', np.int32, n), ('pos', np.int32, n), ('mapq', np.uint8, n), ('flag', np.uint16, n), ('nm', np.int32, n),
            ('l_seq', np.int32, n), ('seq_off', np.int64, n + 1), ('qual_off', np.int64, n + 1), ('cigar_off', np.int64, n + 1),
            ('seq4', np.uint8, sb), ('qual', np.uint8, qb), ('cigar', np.uint32, nc)]
    a = {name: np.asarray(_Column(owner, ptrs[k] or 0, cnt, dt)) for k, (name, dt, cnt) in enumerate(spec[:9 if on_device else 12])}
    refid = a.pop('refid')
    if on_device:
        a.update(seq4=np.zeros(0, np.uint8), qual=np.zeros(0, np.uint8), cigar=np.zeros(0, np.uint32),
                 device=(ptrs[9] or 0, ptrs[10] or 0, ptrs[11] or 0, owner))
    return refid, ReadsSoA(**a)


def _resident_reads(lib, h, owner, n, total):
    """(refid, ResidentReads) of a handle whose records were loaded resident: refID alone is a host column."""
    ptrs = (C.c_void_p * 12)()
    lib.midas_bam_columns(h, ptrs)
    refid = np.asarray(_Column(owner, ptrs[0] or 0, int(n.value), np.int32))
    return refid, ResidentReads(lib, h, owner, int(n.value), int(total.value))


def _decoded(lib, h, load, *args, owner=None, resident=False, on_device=False):
    """What read_bam and read_sam return: load(*args, counts..., err) fills the handle h, then owner -> references -> columns.
    owner: of a handle opened before the load (a load that fails closes it); a load that opens h itself owns it once it
    succeeded.  resident: the load counts (n, sum of l_seq), else (n, SEQ, QUAL, CIGAR)."""
    vals, refs = _i64s(2 if resident else 4)
    host_call(load, *args, *refs)
    owner = owner or _BamOwner(lib, h)
    names, lens = _bam_refs(lib, h)
    if resident:
        return (names, lens) + _resident_reads(lib, h, owner, *vals)
    return (names, lens) + _bam_columns(lib, h, *(int(v.value) for v in vals), owner, on_device=on_device)


def _decoded_resident(lib, load, path, ctx):
    """_decoded for midas_bam_load_resident / midas_sam_load_resident, or None when the payload is more than the resident
    layout addresses (ERR_UNSUPPORTED): the caller goes the columns' way."""
    h = C.c_void_p()
    try:
        return _decoded(lib, h, load, path.encode(), ctx._h, C.byref(h), resident=True)
    except MidasSnpsError as e:
        if e.status != ERR_UNSUPPORTED:
            raise
        return None


def read_bam(path: str, ctx=None, payload_on_device: bool = False, resident: bool = False):
    """Decode a BAM with the native reader -> (ref_names, ref_lengths, refid[int32], ReadsSoA).  The arrays are views of
    the decoder's own buffers (no copy); the native handle lives as long as any of them does.  ctx (a Context): the BGZF
    blocks are inflated on its device instead of by the host's threads (midas_bam_open_device); with payload_on_device SEQ,
    QUAL and CIGAR are also cut out of the inflated stream there and never come down (midas_bam_load_device): the ReadsSoA
    carries their device addresses (`device`) and only that context's batches can take it."""
    lib = load_library()
    h = C.c_void_p()
    if resident:
        # ONE pass from the BAM's bytes to the kernel's input: every column stays on the device, in the direct layout; refID
        # alone comes down (midas_bam_load_resident).  More payload than the layout addresses: the columns' way.
        if not _inflates(ctx):
            raise MidasSnpsError(ERR_INVALID_ARG, "resident needs a device context")
        return _decoded_resident(lib, lib.midas_bam_load_resident, path, ctx) or read_bam(path, ctx, payload_on_device=True)
    if payload_on_device:
        if not _inflates(ctx):
            raise MidasSnpsError(ERR_INVALID_ARG, "payload_on_device needs a device context")
        return _decoded(lib, h, lib.midas_bam_load_device, path.encode(), ctx._h, C.byref(h), on_device=True)
    if _inflates(ctx):
        host_call(lib.midas_bam_open_device, path.encode(), ctx._h, C.byref(h))
    else:
        host_call(lib.midas_bam_open, path.encode(), C.byref(h))
    return _decoded(lib, h, lib.midas_bam_load, h, owner=_BamOwner(lib, h))


class BamDeviceHandle:
    """An open BAM on which nothing is loaded, for Context.genes_count_bam: `ref_names`, `ref_lengths` (the header's, by index)."""

    def __init__(self, lib, h, path):
        self._owner = _BamOwner(lib, h)
        self._h = h
        self.path = path
        self.ref_names, self.ref_lengths = _bam_refs(lib, h)

    def close(self):
        self._owner.__del__()
        self._h = None


def open_bam_device(path: str, ctx) -> BamDeviceHandle:
    """The handle midas_genes_count_bam takes: the file mapped, its block table walked, its header read -- and no record looked at
    (midas_bam_open_share(path, 0, 1, 0): midas_bam_open_device would inflate the whole file to show its header).  ctx: the device
    context the count will run on; without one this raises ERR_INVALID_ARG, there is no host form."""
    if not _inflates(ctx):
        raise MidasSnpsError(ERR_INVALID_ARG, "open_bam_device needs a device context")
    lib = load_library()
    h = C.c_void_p()
    out3 = (C.c_int64 * 3)()
    host_call(lib.midas_bam_open_share, path.encode(), 0, 1, 0, C.byref(h), out3)
    return BamDeviceHandle(lib, h, path)


def read_sam(path: str, ctx=None, order: str = 'coordinate', resident: bool = False):
    """Decode the aligner's SAM text on the device of `ctx` (midas_sam_load_device) -> (ref_names, ref_lengths, refid[int32],
    ReadsSoA), the tuple read_bam(..., payload_on_device=True) returns: the records with a reference, coordinate-sorted there
    (equal keys in file order), the small columns as views of the decoder's host buffers, SEQ / QUAL / CIGAR as device
    addresses (`device`).  order='file': the records stay in the order of their lines (midas_sam_load_device_order; what
    Context.genes_count_device wants).  resident=True (coordinate order only): the sorted records are written once, in the pileup
    kernel's own layout, and every column stays on the device (midas_sam_load_resident) -> (ref_names, ref_lengths, refid,
    ResidentReads), exactly as read_bam(..., resident=True); more payload than that layout addresses: the columns' way.
    There is no host decoder: without a device context this raises ERR_INVALID_ARG."""
    if not _inflates(ctx):
        raise MidasSnpsError(ERR_INVALID_ARG, "read_sam needs a device context (the SAM text is parsed and sorted on the GPU)")
    if order not in SAM_ORDERS:
        raise MidasSnpsError(ERR_INVALID_ARG, "read_sam: order is 'coordinate' or 'file', not %r" % (order,))
    if resident and order != 'coordinate':
        raise MidasSnpsError(ERR_INVALID_ARG, "read_sam: resident records are coordinate-sorted, order=%r is not for them" % (order,))
    lib = load_library()
    if resident:
        return _decoded_resident(lib, lib.midas_sam_load_resident, path, ctx) or read_sam(path, ctx, order)
    h = C.c_void_p()
    if order == 'coordinate':
        return _decoded(lib, h, lib.midas_sam_load_device, path.encode(), ctx._h, C.byref(h), on_device=True)
    return _decoded(lib, h, lib.midas_sam_load_device_order, path.encode(), ctx._h, SAM_ORDERS[order], C.byref(h), on_device=True)


def sam_decode_timing(ctx) -> dict:
    """Host-clock milliseconds of the phases of the context's last read_sam (midas_sam_decode_timing), by name."""
    ms = (C.c_float * 8)()
    st = load_library().midas_sam_decode_timing(ctx._h, ms)
    if st != 0:
        raise MidasSnpsError(st, "midas_sam_decode_timing failed")
    return dict(zip(SAM_PHASES, (float(x) for x in ms)))


class _FastaOwner:
    def __init__(self, lib, h):
        self._lib, self._h = lib, h

    def __del__(self):
        if self._h:
            self._lib.midas_fasta_close(self._h)
            self._h = None


def read_fasta_files(paths, threads: int = 0):
    """The FASTA files `paths` (plain or gzip) read by all cores (midas_fasta_load): (pool, records) -- every sequence back to
    back in one read-only uint8 array (whitespace out, ASCII letters upper-cased), records = [(id, file index, offset, length)]
    in file and record order: what midas_amd/fasta.py parse_bytes yields for each file, `seq.upper()` applied."""
    lib = load_library()
    n = len(paths)
    c_paths = (C.c_char_p * max(n, 1))(*[p.encode() for p in paths])
    h = C.c_void_p()
    host_call(lib.midas_fasta_load, n, c_paths, int(threads), C.byref(h), what="midas_fasta_load")
    owner = _FastaOwner(lib, h)
    nrec = int(lib.midas_fasta_n_records(h))
    ptrs, sizes = (C.c_void_p * 6)(), (C.c_int64 * 2)()
    st = lib.midas_fasta_columns(h, ptrs, sizes)
    if st != 0:
        raise MidasSnpsError(st, "midas_fasta_columns failed")
    pool = np.asarray(_Column(owner, ptrs[0] or 0, int(sizes[0]), np.uint8))
    off = np.asarray(_Column(owner, ptrs[1] or 0, nrec, np.int64))
    ln = np.asarray(_Column(owner, ptrs[2] or 0, nrec, np.int64))
    fi = np.asarray(_Column(owner, ptrs[3] or 0, nrec, np.int32))
    ids = bytes(np.asarray(_Column(owner, ptrs[4] or 0, int(sizes[1]), np.uint8)))
    io = np.asarray(_Column(owner, ptrs[5] or 0, nrec + 1, np.int64))
    recs = [(ids[int(io[k]):int(io[k + 1])].decode('latin-1'), int(fi[k]), int(off[k]), int(ln[k])) for k in range(nrec)]
    return pool, recs


def write_bam(path, ref_names, ref_lengths, refid, reads, level=6, threads=0):
    """The native BAM writer (midas_bam_write): records in the given order, names "r<i>", aux NM + YT:Z:UU -- the bytes of
    midas_amd/bam.py's pure-Python writer, made by all cores."""
    lib = load_library()
    names = (C.c_char_p * len(ref_names))(*[n.encode() for n in ref_names])
    lens = np.ascontiguousarray(ref_lengths, np.int64)
    rid = np.ascontiguousarray(refid, np.int32)
    r = reads._c()
    # (addr: a BAM of no references or no records is still written from its arrays)
    host_call(lib.midas_bam_write, path.encode(), len(ref_names), names, addr(lens), C.byref(r), addr(rid), int(level), int(threads))


class BamSlice:
    """Rank-local view of a BAM (midas_bam_open_slice): this rank's share of the file walked, facts to exchange with the
    other ranks, then only the record ranges this rank owns decoded (midas_bam_load_ranges)."""

    def __init__(self, path: str, slice_index: int, n_slices: int, ctx=None):
        """ctx (a Context): the slice's blocks are inflated and walked on its device (midas_bam_open_slice_device)."""
        self._lib = load_library()
        h = C.c_void_p()
        if _inflates(ctx):
            host_call(self._lib.midas_bam_open_slice_device, path.encode(), int(slice_index), int(n_slices), ctx._h, C.byref(h))
        else:
            host_call(self._lib.midas_bam_open_slice, path.encode(), int(slice_index), int(n_slices), C.byref(h))
        self._h = h
        self.ref_names, self.ref_lens = _bam_refs(self._lib, h)
        n = len(self.ref_names)
        out7 = np.zeros(7, np.int64)
        self.ref_reads, self.ref_bases, self.ref_first = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
        # (addr: a header of no references still hands over its three arrays)
        self._lib.midas_bam_slice_facts(h, ptr(out7), addr(self.ref_reads), addr(self.ref_bases), addr(self.ref_first))
        (self.first, self.end, self.sorted, self.first_ref, self.last_ref, self.rec_begin, self.total) = (int(x) for x in out7)

    def marks(self):
        """(pos_sorted, first_pos, last_pos, ref_span int64 [n_ref], marks int64 [n, 3] = refID, bin, offset): what a
        contig needs to be cut into pieces (midas_bam_slice_marks)."""
        out4 = np.zeros(4, np.int64)
        span = np.zeros(len(self.ref_names), np.int64)
        self._lib.midas_bam_slice_marks(self._h, ptr(out4), addr(span), None, 0)       # (NULL: "not this output")
        marks = np.zeros((int(out4[3]), 3), np.int64)
        if marks.size:
            self._lib.midas_bam_slice_marks(self._h, ptr(out4), None, ptr(marks), marks.shape[0])
        return int(out4[0]), int(out4[1]), int(out4[2]), span, marks

    def _keeper(self):
        keeper = _BamOwner(self._lib, None)
        keeper._slice = self                # the arrays keep this object (and with it the native handle) alive
        return keeper

    def load_ranges(self, ranges, ctx=None, resident: bool = False):
        """[(begin, end)] uncompressed record ranges -> (refid int32, ReadsSoA) of the records in them, in file order.
        ctx (a Context): the ranges are decoded on its device and SEQ / QUAL / CIGAR stay there (midas_bam_load_ranges_device):
        the ReadsSoA carries their device addresses (`device`), as read_bam(..., payload_on_device=True)'s does."""
        rb = np.array([r[0] for r in ranges], np.int64)
        re_ = np.array([r[1] for r in ranges], np.int64)
        lib = self._lib
        if resident and _inflates(ctx) and len(ranges):
            # (everything stays on the device, in the direct layout: read_bam(..., resident=True)'s form for a rank's ranges;
            # ERR_UNSUPPORTED, or a handle that did not go resident: the columns' way below)
            (n, total), refs = _i64s(2)
            try:
                host_call(lib.midas_bam_load_ranges_resident, self._h, ctx._h, len(ranges), ptr(rb), ptr(re_), *refs)
                if lib.midas_bam_is_resident(self._h):
                    return _resident_reads(lib, self._h, self._keeper(), n, total)
            except MidasSnpsError as e:
                if e.status != ERR_UNSUPPORTED:
                    raise
        vals, refs = _i64s(4)
        # (addr: no ranges are two empty arrays and a count of 0)
        if _inflates(ctx):
            host_call(lib.midas_bam_load_ranges_device, self._h, ctx._h, len(ranges), addr(rb), addr(re_), *refs)
        else:
            host_call(lib.midas_bam_load_ranges, self._h, len(ranges), addr(rb), addr(re_), *refs)
        return _bam_columns(lib, self._h, *(int(v.value) for v in vals), self._keeper(),
                            on_device=bool(lib.midas_bam_payload_on_device(self._h)))

    def release_file(self):
        """The ranges are loaded: the file's mapping is unmapped on a thread of its own (midas_bam_release_file)."""
        if getattr(self, '_h', None):
            self._lib.midas_bam_release_file(self._h)

    def close(self):
        if getattr(self, '_h', None):
            self._lib.midas_bam_close(self._h)
            self._h = None

    __del__ = close


class BamShare(BamSlice):
    """A rank's CONTIGUOUS share of a coordinate-sorted BAM (midas_bam_open_share): where this rank's equal share of the file's
    bytes begins, moved forward to the next reference's first record.  `first` (-1: no reference border nearby), `total`,
    `rec_begin`; load_ranges as a slice's -- the one-pass rank-local decode of midas_amd/run/snps.py."""

    def __init__(self, path: str, slice_index: int, n_slices: int, max_walk: int = 256 << 20):
        self._lib = load_library()
        h = C.c_void_p()
        out3 = np.zeros(3, np.int64)
        host_call(self._lib.midas_bam_open_share, path.encode(), int(slice_index), int(n_slices), int(max_walk), C.byref(h), ptr(out3))
        self._h = h
        self.ref_names, self.ref_lens = _bam_refs(self._lib, h)
        self.first, self.total, self.rec_begin = (int(x) for x in out3)

    @classmethod
    def open_local(cls, path: str, slice_index: int, n_slices: int):
        """The share with a LOCAL block table (midas_bam_open_share_local): the rank walks the BGZF chain over its own 1 / N of the
        file only.  `walk` = (first block's file offset, where the walk ended, uncompressed bytes, file size): the ranks exchange
        these, check that they chain, and call locate()."""
        self = cls.__new__(cls)
        self._lib = load_library()
        h = C.c_void_p()
        out4 = np.zeros(4, np.int64)
        host_call(self._lib.midas_bam_open_share_local, path.encode(), int(slice_index), int(n_slices), C.byref(h), ptr(out4))
        self._h, self._slice = h, int(slice_index)
        self.ref_names, self.ref_lens = _bam_refs(self._lib, h)
        self.walk = tuple(int(x) for x in out4)
        self.first = self.total = self.rec_begin = -1
        return self

    def locate(self, upos_base: int, total: int, max_walk: int = 256 << 20):
        out3 = np.zeros(3, np.int64)
        host_call(self._lib.midas_bam_share_locate, self._h, self._slice, int(upos_base), int(total), int(max_walk), ptr(out3))
        self.first, self.total, self.rec_begin = (int(x) for x in out3)
        return self


class _ReadsCalls:
    """Context's part in the decode: the device inflater and the way back from device columns."""

    inflates = True      # read_bam / BamSlice.load_ranges may hand this context the BGZF blocks

    def inflate_blocks(self, comp, cpos, clen, upos, ulen, out_bytes: int, crc=None):
        """Raw DEFLATE streams comp[cpos[k], +clen[k]) -> out[upos[k], +ulen[k]) on the device (midas_snps_inflate_blocks).
        crc: the CRC-32 every stream's inflated bytes must have (None: not checked).
        Raises MidasSnpsError (ERR_BAD_LAYOUT, read_index = the stream) when a stream is corrupt."""
        comp = np.ascontiguousarray(np.frombuffer(comp, np.uint8) if not isinstance(comp, np.ndarray) else comp, dtype=np.uint8)
        cpos, upos = np.ascontiguousarray(cpos, np.int64), np.ascontiguousarray(upos, np.int64)
        clen, ulen = np.ascontiguousarray(clen, np.int32), np.ascontiguousarray(ulen, np.int32)
        out = np.zeros(max(int(out_bytes), 1), np.uint8)
        bad = C.c_int64(-1)
        crc = None if crc is None else np.ascontiguousarray(crc, np.uint32)
        # (addr: no streams are empty arrays and a count of 0; a NULL crc says "not checked")
        st = self._lib.midas_snps_inflate_blocks(self._h, addr(comp), comp.size, cpos.size, addr(cpos), addr(clen), addr(upos), addr(ulen),
                                                 addr(crc), ptr(out), int(out_bytes), C.byref(bad))
        self._check(st, read_index=bad.value)
        return out[:int(out_bytes)]

    def fetch_payload(self, reads: "ReadsSoA") -> "ReadsSoA":
        """A ReadsSoA whose SEQ / QUAL / CIGAR live on the device (read_bam(..., payload_on_device=True)) with those three
        columns copied down: for tests, and for host code that has to slice them."""
        if reads.device is None:
            return reads
        if isinstance(reads, ResidentReads):
            reads = reads.to_columns(self)
        n = reads.n_reads
        sizes = (int(reads.seq_off[n]), int(reads.qual_off[n]), int(reads.cigar_off[n]) * 4)
        out = [np.zeros(max(s, 1), np.uint8) for s in sizes]
        for buf, src, s in zip(out, reads.device[:3], sizes):
            self._check(self._lib.midas_snps_copy_from_device(self._h, ptr(buf), C.c_void_p(int(src)), s))
        d = reads.as_dict()
        d.update(seq4=out[0][:sizes[0]], qual=out[1][:sizes[1]], cigar=out[2][:sizes[2]].view(np.uint32))
        return ReadsSoA(**d)
