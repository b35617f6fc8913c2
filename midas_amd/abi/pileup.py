"""run_midas.py snps: the pileup (one-shot and as a resident Batch), the row coder, and the writers and readers of
<species>.snps.gz."""

from __future__ import annotations

import ctypes as C

import numpy as np

from .core import MidasSnpsError, P, addr, cstr, host_call, i32, i64, load_library, ptr, register, vp
from .reads import ContigTable, ReadsSoA, ResidentReads, _Contigs, _Reads

STAT_ALIGNED_READS, STAT_MAPPED_READS, STAT_COVERED_BASES, STAT_TOTAL_DEPTH = range(4)
NUM_STATS = 4


class Thresholds(C.Structure):
    """scripts/run_midas.py:410-419 defaults."""
    _fields_ = [("baseq", C.c_int32), ("mapq", C.c_int32), ("readq", C.c_int32), ("reserved", C.c_int32),
                ("mapid", C.c_double), ("aln_cov", C.c_double)]

    @classmethod
    def from_args(cls, args: dict) -> "Thresholds":
        return cls(int(args['baseq']), int(args['mapq']), int(args['readq']), 0,
                   float(args['mapid']), float(args['aln_cov']))


DEFAULT_ARGS = {'mapid': 94.0, 'mapq': 20, 'baseq': 30, 'readq': 20, 'aln_cov': 0.75}


class BatchInfo(C.Structure):
    _fields_ = [("n_reads", C.c_int64), ("n_sites", C.c_int64), ("n_tiles", C.c_int64),
                ("packed_bytes", C.c_int64), ("algorithmic_bytes", C.c_int64),
                ("tile_sites", C.c_int32), ("lanes_per_read", C.c_int32), ("n_work_items", C.c_int64),
                ("path", C.c_int32), ("path_auto", C.c_int32), ("lane_bases", C.c_int32), ("layout_build_us", C.c_int32),
                ("direct_general_reads", C.c_int64), ("direct_reach", C.c_int64),
                ("direct_stream_reads", C.c_int64), ("direct_max_tile_reads", C.c_int64),
                ("direct_chunk_tiles", C.c_int32), ("direct_overhang", C.c_int32)]


ROWS_DEVICE, ROWS_HOST = 0, 1    # who formats and deflates a batch's rows (midas_snps_set_row_coder)
PAD_SPEC, PAD_PYSAM = 0, 1       # what the CIGAR op P does to the query position (midas_snps_set_pad_rule)
PATH_AUTO, PATH_DIRECT, PATH_PACKED, PATH_LONG = 0, 1, 2, 3
# midas_snps_batch_fetch_index's out_facts (MIDAS_SNPS_INDEX_* order)
INDEX_FACTS = ('status', 'alg', 'n_general', 'n_long', 'n_outliers', 'max_l', 'max_span', 'max_common', 'unsorted', 'direct_reach',
               'direct_reach_ranges', 'direct_overhang', 'direct_chunks', 'n_outliers_listed', 'outlier_cap')
PATH_NAMES = {PATH_AUTO: "auto", PATH_DIRECT: "direct", PATH_PACKED: "packed", PATH_LONG: "long"}
ROWS_PER_MEMBER = 16384     # MIDAS_SNPS_ROWS_PER_MEMBER: pieces of a contig start at multiples of this

register('exported', {
    'midas_snps_pileup': (i32, [vp, P(Thresholds), P(_Contigs), P(_Reads), vp, vp, vp]),
    'midas_snps_batch_create': (i32, [vp, P(_Contigs), P(_Reads), P(vp)]),
    'midas_snps_batch_create_resident': (i32, [vp, P(_Contigs), vp, i64, P(vp)]),
    'midas_snps_batch_destroy': (None, [vp]),
    'midas_snps_batch_run': (i32, [vp, P(Thresholds)]),
    'midas_snps_batch_sync': (i32, [vp]),
    'midas_snps_batch_fetch': (i32, [vp, vp, vp, vp]),
    'midas_snps_batch_get_info': (i32, [vp, P(BatchInfo)]),
    'midas_snps_batch_enable_timing': (i32, [vp, i32]),
    'midas_snps_batch_timing': (i32, [vp, i32, P(C.c_float)]),
    'midas_snps_batch_time_pileup_only': (i32, [vp, i32]),
    'midas_snps_batch_stats_to_device': (i32, [vp, vp]),
    'midas_snps_batch_pack': (i32, [vp]),
    'midas_snps_batch_select_path': (i32, [vp, i32]),
    'midas_snps_batch_fetch_packed': (i32, [vp, vp, vp, vp, vp, P(i64), P(i64)]),
    'midas_snps_batch_pack_timing': (i32, [vp, i32, P(C.c_float)]),
    'midas_snps_batch_fetch_index': (i32, [vp, vp, vp, vp, vp, vp, vp, P(i64)]),
    'midas_snps_batch_write_part': (i32, [vp, cstr, i32, i32, vp, vp, i32, i32]),
    'midas_snps_set_default_path': (i32, [vp, i32]),
    'midas_snps_set_pad_rule': (i32, [vp, i32]),
    'midas_snps_set_row_coder': (i32, [vp, i32]),
    'midas_snps_row_coder_counts': (i32, [vp, vp]),
    'midas_snps_rows_code': (i32, [vp, i64, vp, vp, i32] + [vp] * 6 + [i64, i64, i32] + [vp] * 6 + [i64, P(i64)]),
    'midas_snps_deflate_rows': (i32, [vp, i64, vp, vp, i64, vp, i64, P(i64)]),
    'midas_snps_write_rows': (i32, [cstr, i32, cstr, i64, vp, vp, i32, i32, cstr]),
    'midas_snps_write_table': (i32, [cstr, i32, vp, vp, vp, vp, i32, i32, cstr]),
    'midas_snps_write_part': (i32, [cstr, i32, i32, vp, vp, vp, vp, i32, i32, cstr]),
    'midas_snps_write_pieces': (i32, [cstr, i32, i32, vp, vp, vp, vp, vp, i32, i32, cstr]),
    'midas_snps_table_open': (i32, [cstr, i64, i32, P(vp), cstr]),
    'midas_snps_table_open_range': (i32, [cstr, i64, i64, i32, P(vp), cstr]),
    'midas_snps_table_count_rows': (i32, [cstr, P(i64), cstr]),
    'midas_snps_table_close': (None, [vp]),
    'midas_snps_table_rows': (i64, [vp]),
    'midas_snps_table_key_bytes': (i64, [vp]),
    'midas_snps_table_copy': (i32, [vp, vp, vp, vp]),
    'midas_snps_tableset_open': (i32, [i32, vp, P(vp), vp, cstr]),
    'midas_snps_tableset_read_counts': (i32, [vp, i64, i64, vp, cstr]),
    'midas_snps_tableset_close': (None, [vp]),
})


def deflate_rows(text: bytes, row_begin, tail_begin) -> bytes:
    """Raw DEFLATE stream of row-structured text by the library's row coder (midas_snps_deflate_rows)."""
    lib = load_library()
    buf = np.frombuffer(text, dtype=np.uint8)
    rb = np.ascontiguousarray(row_begin, dtype=np.uint32)
    tb = np.ascontiguousarray(tail_begin, dtype=np.uint32)
    out = np.empty(len(text) + len(text) // 8 + 4096, dtype=np.uint8)
    n_out = C.c_int64(0)
    st = lib.midas_snps_deflate_rows(buf.ctypes.data, len(text), rb.ctypes.data, tb.ctypes.data, rb.size, out.ctypes.data,
                                     out.size, C.byref(n_out))
    if st != 0:
        raise MidasSnpsError(st, "midas_snps_deflate_rows: bad row offsets or output too small")
    return out[:n_out.value].tobytes()


def write_rows(path: str, append: bool, ref_id: str, allele: np.ndarray, counts: np.ndarray,
               gz_level: int = 4, threads: int = 0):
    """Format + gzip the rows of ONE contig into <species>.snps.gz (midas_snps_write_rows)."""
    lib = load_library()
    allele = np.ascontiguousarray(allele, dtype=np.uint8)
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    assert counts.shape == (allele.shape[0], 4)
    # (addr: a contig of no rows is still written, from its arrays)
    host_call(lib.midas_snps_write_rows, path.encode(), 1 if append else 0, ref_id.encode(), allele.shape[0],
              addr(allele), addr(counts), int(gz_level), int(threads))


def write_table(path: str, ref_ids, alleles, counts, gz_level: int = 4, threads: int = 0, header=None, first_pos=None):
    """Header + the rows of every contig of one species in one call (midas_snps_write_table): ref_ids[k],
    alleles[k] (u8[n_k]) and counts[k] (u32[n_k,4]) describe contig k in output order.  header = True / False writes a
    PART of a species' table instead (midas_snps_write_part): with or without the header member in front.  first_pos:
    the entries are pieces of contigs, entry k's first row is position first_pos[k] + 1 (midas_snps_write_pieces)."""
    lib = load_library()
    n = len(ref_ids)
    al = [np.ascontiguousarray(a, dtype=np.uint8) for a in alleles]
    cn = [np.ascontiguousarray(c, dtype=np.uint32) for c in counts]
    assert all(c.shape == (a.shape[0], 4) for a, c in zip(al, cn))
    ids = (C.c_char_p * max(n, 1))(*[r.encode() for r in ref_ids])
    ns = (C.c_int64 * max(n, 1))(*[a.shape[0] for a in al])
    pa = (C.c_void_p * max(n, 1))(*[a.ctypes.data for a in al])
    pc = (C.c_void_p * max(n, 1))(*[c.ctypes.data for c in cn])
    if first_pos is not None:
        fp = (C.c_int64 * max(n, 1))(*[int(x) for x in first_pos])
        host_call(lib.midas_snps_write_pieces, path.encode(), 1 if (header is None or header) else 0, n, ids, ns, fp, pa, pc,
                  int(gz_level), int(threads))
    elif header is None:
        host_call(lib.midas_snps_write_table, path.encode(), n, ids, ns, pa, pc, int(gz_level), int(threads))
    else:
        host_call(lib.midas_snps_write_part, path.encode(), 1 if header else 0, n, ids, ns, pa, pc, int(gz_level), int(threads))


def count_snps_rows(path: str) -> int:
    """Rows of a <species>.snps.gz without inflating it, or -1 when the file does not say (midas_snps_table_count_rows)."""
    lib = load_library()
    n = C.c_int64(-1)
    host_call(lib.midas_snps_table_count_rows, path.encode(), C.byref(n))
    return int(n.value)


def read_snps_table(path: str, max_rows: int = -1, want_keys: bool = True, row_begin: int = 0):
    """Parse one <species>.snps.gz with the native reader -> (counts[n,4] u32, keys | None, key_off | None);
    keys is a byte buffer, row i's 'ref_id|ref_pos|ref_allele' is bytes(keys[key_off[i]:key_off[i + 1]]).
    Rows [row_begin, max_rows) of the table (max_rows < 0: to the end)."""
    lib = load_library()
    h = C.c_void_p()
    host_call(lib.midas_snps_table_open_range, path.encode(), int(row_begin), int(max_rows), 1 if want_keys else 0, C.byref(h))
    try:
        n = int(lib.midas_snps_table_rows(h))
        counts = np.empty((n, 4), np.uint32)
        keys = np.empty(int(lib.midas_snps_table_key_bytes(h)), np.uint8) if want_keys else None
        key_off = np.empty(n + 1, np.int64) if want_keys else None
        lib.midas_snps_table_copy(h, addr(counts), addr(keys), addr(key_off))      # (NULL: the keys are not wanted)
    finally:
        lib.midas_snps_table_close(h)
    return counts, (memoryview(keys) if want_keys else None), key_off


class _TableSet:
    """Several samples' <species>.snps.gz opened as one set (midas_snps_tableset_open): .rows int64 per table, -1 for a file
    that does not announce its rows; rows(row_begin, max_rows) = how many the SHORTEST table has in that range."""

    def __init__(self, lib, paths):
        self._lib, self.n = lib, len(paths)
        arr = (C.c_char_p * self.n)(*[p.encode() for p in paths])
        self.rows = np.empty(self.n, np.int64)
        self.h = C.c_void_p()
        host_call(lib.midas_snps_tableset_open, self.n, arr, C.byref(self.h), addr(self.rows))

    def count(self, row_begin: int, max_rows: int) -> int:
        hi = int(self.rows.min()) if max_rows < 0 else min(int(self.rows.min()), int(max_rows))
        return max(0, hi - int(row_begin))

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self._lib.midas_snps_tableset_close(self.h)


def read_snps_counts(paths, row_begin: int = 0, max_rows: int = -1):
    """The count columns of several samples' <species>.snps.gz in one parallel region (midas_snps_tableset_*):
    -> list of counts[n,4] u32, one per path, n = rows [row_begin, max_rows) of the SHORTEST table (max_rows < 0: its
    end) -- the reference's zip over the samples' files stops there too.  None when one of the files does not announce
    its rows (written by the reference): read those with read_snps_table."""
    lib = load_library()
    with _TableSet(lib, paths) as ts:
        if (ts.rows < 0).any():
            return None
        m = ts.count(row_begin, max_rows)
        out = [np.empty((m, 4), np.uint32) for _ in range(ts.n)]
        ptrs = (C.c_void_p * ts.n)(*[a.ctypes.data for a in out])
        host_call(lib.midas_snps_tableset_read_counts, ts.h, int(row_begin), m, ptrs)
        return out


class _PileupCalls:
    """Context's pileup commands and the settings of the batches made on it."""

    def set_default_path(self, path: int):
        """The path of every batch created on this context from now on (PATH_AUTO: each batch's own choice)."""
        self._check(self._lib.midas_snps_set_default_path(self._h, int(path)))

    def set_pad_rule(self, rule: int):
        """PAD_SPEC (default): the CIGAR op P consumes nothing; PAD_PYSAM: it advances the query position, as
        get_aligned_pairs of the pysam releases of MIDAS's time does.  For batches created afterwards."""
        self._check(self._lib.midas_snps_set_pad_rule(self._h, int(rule)))

    def set_row_coder(self, coder: int):
        """ROWS_DEVICE (default): Batch.write_part formats and deflates the rows in a kernel; ROWS_HOST: the host's
        formatter threads do (the file then equals write_table's byte for byte).  Same text either way."""
        self._check(self._lib.midas_snps_set_row_coder(self._h, int(coder)))

    def row_coder_counts(self):
        """Who coded the parts Batch.write_part wrote on this context (midas_snps_row_coder_counts): members coded by the kernel,
        parts left to the host's formatter for a contig id beyond 192 bytes, parts left to it for a member the kernel declined."""
        out = np.zeros(3, np.int64)
        self._check(self._lib.midas_snps_row_coder_counts(self._h, ptr(out)))
        return {"members_on_device": int(out[0]), "parts_declined_id": int(out[1]), "parts_declined_status": int(out[2])}

    def rows_code(self, counts, allele, members, arena_bytes: int = 0, grid_blocks: int = 0):
        """The row kernel's launch of Batch.write_part on chosen inputs (midas_snps_rows_code).  counts [n_sites, 4] uint32,
        allele [n_sites] uint8 (any byte), members: (site0, pos0, n_rows, id bytes) each, handed to the kernel as given;
        arena_bytes 0: the product's rule, grid_blocks 0: one workgroup per compute unit.
        -> one dict per member: status, n_bytes, crc, text_len, arena_off, stream (bytes; None unless status 0)."""
        counts = np.ascontiguousarray(counts, np.uint32).reshape(-1, 4)
        allele = np.ascontiguousarray(allele, np.uint8).reshape(-1)
        n = len(members)
        site0 = np.array([m[0] for m in members], np.int64)
        pos0 = np.array([m[1] for m in members], np.int64)
        n_rows = np.array([m[2] for m in members], np.int32)
        id_len = np.array([len(m[3]) for m in members], np.int32)
        id_off = (np.cumsum(id_len, dtype=np.int64) - id_len).astype(np.int32)
        ids = np.frombuffer(b"".join(bytes(m[3]) for m in members) + b"\0", np.uint8)
        rows = int(np.clip(n_rows.astype(np.int64), 0, 16384).sum())
        cap = int(arena_bytes) if arena_bytes else rows * 10 + n * 1024 + 4096
        st_, nb, crc, tl = (np.zeros(max(n, 1), np.uint32) for _ in range(4))
        off = np.zeros(max(n, 1), np.int64)
        streams = np.zeros(cap + 16, np.uint8)
        got = C.c_int64(0)
        # (addr: the kernel is handed what the test chose, no sites or no members included)
        self._check(self._lib.midas_snps_rows_code(self._h, allele.size, addr(counts), addr(allele), n, addr(site0), addr(pos0),
                                                   addr(n_rows), addr(id_off), addr(id_len), ptr(ids), ids.size - 1, int(arena_bytes),
                                                   int(grid_blocks), ptr(st_), ptr(nb), ptr(crc), ptr(tl), ptr(off), ptr(streams),
                                                   streams.size, C.byref(got)))
        out, at = [], 0
        for k in range(n):
            stream = None
            if st_[k] == 0:
                stream = streams[at:at + int(nb[k])].tobytes()
                at += int(nb[k])
            out.append(dict(status=int(st_[k]), n_bytes=int(nb[k]), crc=int(crc[k]), text_len=int(tl[k]), arena_off=int(off[k]), stream=stream))
        assert at == got.value
        return out

    def pileup(self, thr: Thresholds, contigs: ContigTable, reads: ReadsSoA, want_allele: bool = True, pinned_slot=None):
        """One-shot midas_snps_pileup(): returns (counts[n_sites,4] u32, allele[n_sites] u8 | None, stats[n_species,4] i64).
        pinned_slot: the per-site results land in the context's page-locked buffers of that name (one DMA, no staging)
        and stay valid until the next call with the same slot."""
        n = contigs.n_sites
        if pinned_slot is None:
            counts = np.empty((n, 4), dtype=np.uint32)
            allele = np.empty(n, dtype=np.uint8) if want_allele else None
        else:
            counts = self.pinned(('counts', pinned_slot), (n, 4), np.uint32)
            allele = self.pinned(('allele', pinned_slot), (n,), np.uint8) if want_allele else None
        stats = np.zeros((contigs.n_species, NUM_STATS), dtype=np.int64)
        c, r = contigs._c(), reads._c()
        # (addr: a NULL allele says "not wanted"; tables of no sites or no species keep their addresses)
        st = self._lib.midas_snps_pileup(self._h, C.byref(thr), C.byref(c), C.byref(r), addr(counts), addr(allele), addr(stats))
        self._check(st)
        return counts, allele, stats

    def batch(self, contigs: ContigTable, reads: ReadsSoA) -> "Batch":
        return Batch(self, contigs, reads)


class Batch:
    """Device-resident (contig table, reads): upload once, run many."""

    def __init__(self, ctx: Context, contigs: ContigTable, reads: ReadsSoA):
        self.ctx = ctx
        self._lib = ctx._lib
        self.n_sites = contigs.n_sites
        self.n_species = int(contigs.n_species)
        h = C.c_void_p()
        c = contigs._c()
        if isinstance(reads, ResidentReads):       # the handle's records where they lie (and the handle alive as long as the batch)
            self._keep = reads.owner
            ctx._check(self._lib.midas_snps_batch_create_resident(ctx._h, C.byref(c), reads._h, reads.first, C.byref(h)))
        else:
            r = reads._c()
            ctx._check(self._lib.midas_snps_batch_create(ctx._h, C.byref(c), C.byref(r), C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, '_h', None):
            self._lib.midas_snps_batch_destroy(self._h)
            self._h = None

    __del__ = close

    def run(self, thr: Thresholds):
        self.ctx._check(self._lib.midas_snps_batch_run(self._h, C.byref(thr)))
        if getattr(self, '_slots', 0):
            self._timed += 1

    def sync(self):
        self.ctx._check(self._lib.midas_snps_batch_sync(self._h))

    def fetch(self, counts: bool = True, allele: bool = True, stats: bool = True):
        oc = np.empty((self.n_sites, 4), dtype=np.uint32) if counts else None
        oa = np.empty(self.n_sites, dtype=np.uint8) if allele else None
        os_ = np.zeros((self.n_species, NUM_STATS), dtype=np.int64) if stats else None
        self.ctx._check(self._lib.midas_snps_batch_fetch(self._h, addr(oc), addr(oa), addr(os_)))     # (NULL: "not this output")
        return oc, oa, os_

    def write_part(self, path: str, contig_index, ref_ids, header: bool = True, gz_level: int = 4, threads: int = 0):
        """Rows of the contigs contig_index (indices into the batch's contig table, output order) straight from the device
        results into a gzip table or part of one (midas_snps_batch_write_part)."""
        n = len(contig_index)
        idx = np.ascontiguousarray(contig_index, dtype=np.int32)
        ids = (C.c_char_p * max(n, 1))(*[r.encode() for r in ref_ids])
        # (addr: a part of no contigs, the header alone, is a valid call)
        self.ctx._check(self._lib.midas_snps_batch_write_part(self._h, path.encode(), 1 if header else 0, n,
                                                              addr(idx), ids, int(gz_level), int(threads)))

    def info(self) -> BatchInfo:
        bi = BatchInfo()
        self.ctx._check(self._lib.midas_snps_batch_get_info(self._h, C.byref(bi)))
        return bi

    def enable_timing(self, n_slots: int = 1):
        """n_slots event triples; run k records into slot k % n_slots (0 turns timing off)."""
        self.ctx._check(self._lib.midas_snps_batch_enable_timing(self._h, int(n_slots)))
        self._slots = int(n_slots)
        self._timed = 0
        self._packs = 0

    def time_pileup_only(self, on: bool = True):
        """Timed runs record only the two events around the pileup kernel (index_ms reads 0, run_ms == pileup_ms)."""
        self.ctx._check(self._lib.midas_snps_batch_time_pileup_only(self._h, 1 if on else 0))

    def timing(self, slot: int = 0):
        ms = (C.c_float * 3)()
        self.ctx._check(self._lib.midas_snps_batch_timing(self._h, int(slot), ms))
        return {'index_ms': ms[0], 'pileup_ms': ms[1], 'run_ms': ms[2]}

    def last_timing(self):
        return self.timing((self._timed - 1) % self._slots)

    def select_path(self, path: int):
        """PATH_DIRECT: the pileup kernel reads the raw arrays; PATH_PACKED: tile-ordered records + payload; PATH_AUTO: the
        batch's own choice (midas_snps_batch_select_path)."""
        self.ctx._check(self._lib.midas_snps_batch_select_path(self._h, int(path)))

    def pack(self):
        """Re-run the device packer over the resident raw reads (midas_snps_batch_pack)."""
        self.ctx._check(self._lib.midas_snps_batch_pack(self._h))
        if getattr(self, '_slots', 0):
            self._packs += 1

    def pack_timing(self, slot: int = 0):
        ms = (C.c_float * 2)()
        self.ctx._check(self._lib.midas_snps_batch_pack_timing(self._h, int(slot), ms))
        return {'pack_ms': ms[0], 'scatter_ms': ms[1]}

    def fetch_packed(self):
        """The device-packed layout: (rec[n_records+1,16] u8 incl. the sentinel, blob u8, orig u32, key u32)."""
        n, nb = C.c_int64(0), C.c_int64(0)
        self.ctx._check(self._lib.midas_snps_batch_fetch_packed(self._h, None, None, None, None, C.byref(n), C.byref(nb)))
        rec = np.zeros((n.value + 1, 16), np.uint8)
        blob = np.zeros(max(nb.value, 1), np.uint8)
        orig = np.zeros(max(n.value, 1), np.uint32)
        key = np.zeros(max(n.value, 1), np.uint32)
        self.ctx._check(self._lib.midas_snps_batch_fetch_packed(self._h, ptr(rec), ptr(blob), ptr(orig), ptr(key), C.byref(n), C.byref(nb)))
        return rec, blob[:nb.value], orig[:n.value], key[:n.value]

    def fetch_index(self):
        """One ranges pass of the direct path on the batch's current parity, and what the index pass left on the device
        (midas_snps_batch_fetch_index; test aid): a dict of tbegin / tend [n_tiles] u32, facts {name: int} in INDEX_FACTS order,
        outliers [n_listed, 3] u32 (read, first tile, last tile; device order), tile_flag [n_tiles] u8 and chunk_ok u8 (empty when
        the batch has no such table)."""
        bi = self.info()
        nt, cap = int(bi.n_tiles), max(4096, int(bi.n_reads) // 64)
        tb, te = np.zeros(max(nt, 1), np.uint32), np.zeros(max(nt, 1), np.uint32)
        facts = np.zeros(len(INDEX_FACTS), np.int64)
        out3 = np.zeros((cap, 3), np.uint32)
        flag, ok = np.zeros(max(nt, 1), np.uint8), np.zeros(max(nt // 4, 1), np.uint8)
        n_ok = C.c_int64(0)
        self.ctx._check(self._lib.midas_snps_batch_fetch_index(self._h, ptr(tb), ptr(te), ptr(facts), ptr(out3), ptr(flag), ptr(ok),
                                                               C.byref(n_ok)))
        f = dict(zip(INDEX_FACTS, (int(x) for x in facts)))
        return dict(tbegin=tb[:nt], tend=te[:nt], facts=f, outliers=out3[:min(f['n_outliers_listed'], cap)].copy(), tile_flag=flag[:nt],
                    chunk_ok=ok[:n_ok.value].copy())

    def stats_to_device(self, dst_device_ptr: int):
        """Enqueue a D2D copy of the [n_species,4] int64 counters into caller-owned device memory."""
        self.ctx._check(self._lib.midas_snps_batch_stats_to_device(self._h, C.c_void_p(dst_device_ptr)))
