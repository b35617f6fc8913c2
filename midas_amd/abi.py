"""ctypes binding of include/midas_snps.h (libmidas_snps_hip.so).

There is no CPU fallback: if the library is missing, or no gfx950 GPU is visible,
the calls raise.  Nothing under ``oracle/`` is imported from here.
"""

from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

from . import build as _build

ABI_VERSION = 4

STAT_ALIGNED_READS, STAT_MAPPED_READS, STAT_COVERED_BASES, STAT_TOTAL_DEPTH = range(4)
NUM_STATS = 4

ERR_READ_NO_SEQ, ERR_READ_NO_NM, ERR_READ_ZERO_ALIGN, ERR_READ_NO_QUAL, ERR_READ_CIGAR_OVERRUN, \
    ERR_READ_BAD_CIGAR_OP = range(1, 7)
ERR_INVALID_ARG, ERR_NO_DEVICE, ERR_HIP, ERR_OUT_OF_MEMORY, ERR_UNSUPPORTED, ERR_BAD_LAYOUT = \
    -1, -2, -3, -4, -5, -6


class MidasSnpsError(RuntimeError):
    def __init__(self, status: int, message: str, read_index: int = -1):
        super().__init__("midas_snps status %d: %s" % (status, message))
        self.status = status
        self.message = message
        self.read_index = read_index


class Thresholds(C.Structure):
    """scripts/run_midas.py:410-419 defaults."""
    _fields_ = [("baseq", C.c_int32), ("mapq", C.c_int32), ("readq", C.c_int32), ("reserved", C.c_int32),
                ("mapid", C.c_double), ("aln_cov", C.c_double)]

    @classmethod
    def from_args(cls, args: dict) -> "Thresholds":
        return cls(int(args['baseq']), int(args['mapq']), int(args['readq']), 0,
                   float(args['mapid']), float(args['aln_cov']))


DEFAULT_ARGS = {'mapid': 94.0, 'mapq': 20, 'baseq': 30, 'readq': 20, 'aln_cov': 0.75}

ERR_MERGE_ZERO_MEAN_DEPTH = 7
SNP_TYPE_BITS = {'any': 1, 'mono': 2, 'bi': 4, 'tri': 8, 'quad': 16}
SNP_TYPE_NAMES = [None, 'mono', 'bi', 'tri', 'quad']


class MergeParams(C.Structure):
    """scripts/merge_midas.py:229-252 (site filters) as the kernel takes them."""
    _fields_ = [("allele_freq", C.c_double), ("site_ratio", C.c_double), ("site_prev", C.c_double),
                ("site_depth", C.c_int32), ("snp_types", C.c_int32)]

    @classmethod
    def from_args(cls, args: dict) -> "MergeParams":
        bits = 0
        for t in args['snp_type']:
            bits |= SNP_TYPE_BITS[t]
        return cls(float(args['allele_freq']), float(args['site_ratio']), float(args['site_prev']),
                   int(args['site_depth']), bits)


DEFAULT_MERGE_ARGS = {'snp_type': ['bi'], 'allele_freq': 0.01, 'site_depth': 1, 'site_ratio': 2.0, 'site_prev': 0.95}


class _Reads(C.Structure):
    _fields_ = [("n_reads", C.c_int64), ("pos", C.c_void_p), ("mapq", C.c_void_p), ("flag", C.c_void_p),
                ("nm", C.c_void_p), ("l_seq", C.c_void_p), ("seq_off", C.c_void_p), ("qual_off", C.c_void_p),
                ("cigar_off", C.c_void_p), ("seq4", C.c_void_p), ("qual", C.c_void_p), ("cigar", C.c_void_p)]


class _Contigs(C.Structure):
    _fields_ = [("n_contigs", C.c_int32), ("n_species", C.c_int32), ("length", C.c_void_p),
                ("species", C.c_void_p), ("read_begin", C.c_void_p), ("ref", C.c_void_p), ("origin", C.c_void_p)]


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
        p = lambda a: a.ctypes.data_as(C.c_void_p)   # zero-size arrays still have a valid address
        payload = (p(self.seq4), p(self.qual), p(self.cigar)) if self.device is None else \
            tuple(C.c_void_p(int(x)) for x in self.device[:3])
        return _Reads(self.n_reads, p(self.pos), p(self.mapq), p(self.flag), p(self.nm), p(self.l_seq),
                      self.seq_off.ctypes.data_as(C.c_void_p), self.qual_off.ctypes.data_as(C.c_void_p),
                      self.cigar_off.ctypes.data_as(C.c_void_p), *payload)


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
        err = C.create_string_buffer(256)
        st = self._lib.midas_bam_resident_to_columns(self._h, ctx._h, C.byref(sb), C.byref(qb), C.byref(nc), err)
        if st != 0:
            raise MidasSnpsError(st, err.value.decode())
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
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        return _Contigs(self.n_contigs, int(self.n_species), p(self.length), p(self.species),
                        self.read_begin.ctypes.data_as(C.c_void_p), p(self.ref), p(self.origin) if self.origin is not None else None)


_lib = None


def library_path() -> str:
    return _build.LIB_PATH


def load_library(build_if_missing: bool = True):
    """dlopen the in-tree libmidas_snps_hip.so; raises if it cannot be found or built."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("MIDAS_SNPS_LIBRARY") or _build.LIB_PATH     # override: developer builds (tools/)
    if not os.path.exists(path):
        if not build_if_missing:
            raise MidasSnpsError(ERR_NO_DEVICE, "native library %s is missing (run `python -m midas_amd.build`)" % path)
        _build.build_native()
    lib = C.CDLL(path)
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    sig = {
        'midas_snps_abi_version': (i32, []),
        'midas_snps_cpu_budget': (i32, []),
        'midas_snps_status_string': (C.c_char_p, [i32]),
        'midas_snps_create': (i32, [i32, C.POINTER(vp)]),
        'midas_snps_destroy': (None, [vp]),
        'midas_snps_last_error': (C.c_char_p, [vp]),
        'midas_snps_last_error_read': (i64, [vp]),
        'midas_snps_set_stream': (i32, [vp, vp]),
        'midas_snps_device_info': (i32, [vp, C.c_char_p, C.POINTER(i32), C.POINTER(i64)]),
        'midas_snps_host_alloc': (vp, [i64]),
        'midas_snps_host_free': (None, [vp]),
        'midas_snps_pileup': (i32, [vp, C.POINTER(Thresholds), C.POINTER(_Contigs), C.POINTER(_Reads), vp, vp, vp]),
        'midas_snps_batch_create': (i32, [vp, C.POINTER(_Contigs), C.POINTER(_Reads), C.POINTER(vp)]),
        'midas_snps_batch_destroy': (None, [vp]),
        'midas_snps_batch_run': (i32, [vp, C.POINTER(Thresholds)]),
        'midas_snps_batch_sync': (i32, [vp]),
        'midas_snps_batch_fetch': (i32, [vp, vp, vp, vp]),
        'midas_snps_batch_get_info': (i32, [vp, C.POINTER(BatchInfo)]),
        'midas_snps_batch_enable_timing': (i32, [vp, i32]),
        'midas_snps_batch_timing': (i32, [vp, i32, C.POINTER(C.c_float)]),
        'midas_snps_batch_time_pileup_only': (i32, [vp, i32]),
        'midas_snps_batch_stats_to_device': (i32, [vp, vp]),
        'midas_snps_batch_pack': (i32, [vp]),
        'midas_snps_batch_select_path': (i32, [vp, i32]),
        'midas_snps_set_default_path': (i32, [vp, i32]),
        'midas_snps_set_pad_rule': (i32, [vp, i32]),
        'midas_snps_stream_rates': (i32, [vp, i64, i32, C.POINTER(C.c_double)]),
        'midas_snps_calibration_pass': (i32, [vp, i64]),
        'midas_snps_set_row_coder': (i32, [vp, i32]),
        'midas_snps_row_coder_counts': (i32, [vp, vp]),
        'midas_snps_rows_code': (i32, [vp, i64, vp, vp, i32] + [vp] * 6 + [i64, i64, i32] + [vp] * 6 + [i64, C.POINTER(i64)]),
        'midas_snps_scan_u32': (i32, [vp, i64, vp, i32, vp, C.POINTER(i32), C.POINTER(i32)]),
        'midas_snps_sort_pairs': (i32, [vp, i64, i32, i32, vp, vp, vp, vp, C.POINTER(i32), C.POINTER(i32)]),
        'midas_snps_copy_rate': (i32, [vp, i64, i32, C.POINTER(C.c_double)]),
        'midas_snps_batch_fetch_packed': (i32, [vp, vp, vp, vp, vp, C.POINTER(i64), C.POINTER(i64)]),
        'midas_snps_batch_pack_timing': (i32, [vp, i32, C.POINTER(C.c_float)]),
        'midas_snps_batch_fetch_index': (i32, [vp, vp, vp, vp, vp, vp, vp, C.POINTER(i64)]),
    }
    sig.update({
        'midas_bam_open': (i32, [C.c_char_p, C.POINTER(vp), C.c_char_p]),
        'midas_bam_close': (None, [vp]),
        'midas_bam_write': (i32, [C.c_char_p, i32, C.POINTER(C.c_char_p), vp, C.POINTER(_Reads), vp, i32, i32, C.c_char_p]),
        'midas_bam_n_refs': (i32, [vp]),
        'midas_bam_ref': (i32, [vp, i32, C.POINTER(C.c_char_p), C.POINTER(i64)]),
        'midas_bam_load': (i32, [vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64), C.POINTER(i64), C.c_char_p]),
        'midas_bam_copy': (i32, [vp] + [vp] * 12),
        'midas_bam_columns': (i32, [vp, vp]),
        'midas_bam_open_slice': (i32, [C.c_char_p, i32, i32, C.POINTER(vp), C.c_char_p]),
        'midas_bam_slice_facts': (i32, [vp, vp, vp, vp, vp]),
        'midas_bam_slice_marks': (i32, [vp, vp, vp, vp, C.c_int64]),
        'midas_bam_open_device': (i32, [C.c_char_p, vp, C.POINTER(vp), C.c_char_p]),
        'midas_bam_open_slice_device': (i32, [C.c_char_p, i32, i32, vp, C.POINTER(vp), C.c_char_p]),
        'midas_bam_load_device': (i32, [C.c_char_p, vp, C.POINTER(vp), C.POINTER(i64), C.POINTER(i64), C.POINTER(i64), C.POINTER(i64), C.c_char_p]),
        'midas_bam_payload_on_device': (i32, [vp]),
        'midas_sam_load_device': (i32, [C.c_char_p, vp, C.POINTER(vp), C.POINTER(i64), C.POINTER(i64), C.POINTER(i64), C.POINTER(i64), C.c_char_p]),
        'midas_sam_decode_timing': (i32, [vp, vp]),
        'midas_sam_load_device_order': (i32, [C.c_char_p, vp, i32, C.POINTER(vp), C.POINTER(i64), C.POINTER(i64), C.POINTER(i64), C.POINTER(i64), C.c_char_p]),
        'midas_sam_load_resident': (i32, [C.c_char_p, vp, C.POINTER(vp), C.POINTER(i64), C.POINTER(i64), C.c_char_p]),
        'midas_bam_release_file': (None, [vp]),
        'midas_bam_load_resident': (i32, [C.c_char_p, vp, C.POINTER(vp), C.POINTER(i64), C.POINTER(i64), C.c_char_p]),
        'midas_bam_load_ranges_resident': (i32, [vp, vp, i32, vp, vp, C.POINTER(i64), C.POINTER(i64), C.c_char_p]),
        'midas_bam_is_resident': (i32, [vp]),
        'midas_bam_open_share_local': (i32, [C.c_char_p, i32, i32, C.POINTER(vp), vp, C.c_char_p]),
        'midas_bam_share_locate': (i32, [vp, i32, i64, i64, i64, vp, C.c_char_p]),
        'midas_bam_resident_to_columns': (i32, [vp, vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64), C.c_char_p]),
        'midas_snps_batch_create_resident': (i32, [vp, C.POINTER(_Contigs), vp, i64, C.POINTER(vp)]),
        'midas_snps_copy_from_device': (i32, [vp, vp, vp, i64]),
        'midas_bam_load_ranges_device': (i32, [vp, vp, i32, vp, vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64), C.POINTER(i64), C.c_char_p]),
        'midas_snps_inflate_blocks': (i32, [vp, vp, i64, i64, vp, vp, vp, vp, vp, vp, i64, C.POINTER(i64)]),
        'midas_bam_load_ranges': (i32, [vp, i32, vp, vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64), C.POINTER(i64), C.c_char_p]),
        'midas_snps_write_rows': (i32, [C.c_char_p, i32, C.c_char_p, i64, vp, vp, i32, i32, C.c_char_p]),
        'midas_merge_write_info': (i32, [C.c_char_p, C.c_char_p, i64, vp, vp, vp, vp, vp, vp, vp, i32, i64, C.c_char_p]),
        'midas_merge_write_matrix': (i32, [C.c_char_p, C.c_char_p, i64, vp, i32, i64, vp, vp, i32, i64, C.c_char_p]),
        'midas_merge_write_matrix_device': (i32, [vp, C.c_char_p, C.c_char_p, i64, vp, i32, i64, vp, vp, i64, C.POINTER(C.c_float)]),
        'midas_merge_sites_tables': (i32, [vp, C.POINTER(MergeParams), i32, i64, C.POINTER(vp), vp, C.c_char_p, C.c_char_p, C.c_char_p, i64,
                                           vp, vp, vp, C.POINTER(i64), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
        'midas_snps_table_open_range': (i32, [C.c_char_p, i64, i64, i32, C.POINTER(vp), C.c_char_p]),
        'midas_snps_table_count_rows': (i32, [C.c_char_p, C.POINTER(i64), C.c_char_p]),
        'midas_snps_write_table': (i32, [C.c_char_p, i32, vp, vp, vp, vp, i32, i32, C.c_char_p]),
        'midas_snps_write_part': (i32, [C.c_char_p, i32, i32, vp, vp, vp, vp, i32, i32, C.c_char_p]),
        'midas_snps_write_pieces': (i32, [C.c_char_p, i32, i32, vp, vp, vp, vp, vp, i32, i32, C.c_char_p]),
        'midas_snps_deflate_rows': (i32, [vp, i64, vp, vp, i64, vp, i64, C.POINTER(i64)]),
        'midas_snps_batch_write_part': (i32, [vp, C.c_char_p, i32, i32, vp, vp, i32, i32]),
        'midas_fasta_load': (i32, [i32, vp, i32, C.POINTER(vp), C.c_char_p]),
        'midas_fasta_n_records': (i64, [vp]),
        'midas_fasta_columns': (i32, [vp, vp, vp]),
        'midas_fasta_close': (None, [vp]),
        'midas_snps_tableset_open': (i32, [i32, vp, C.POINTER(vp), vp, C.c_char_p]),
        'midas_snps_tableset_read_counts': (i32, [vp, i64, i64, vp, C.c_char_p]),
        'midas_snps_tableset_close': (None, [vp]),
        'midas_merge_tables_create': (i32, [vp, i32, i64, C.POINTER(vp)]),
        'midas_merge_tables_free': (None, [vp]),
        'midas_merge_tables_shape': (i32, [vp, C.POINTER(i32), C.POINTER(i64)]),
        'midas_merge_tables_set_host': (i32, [vp, vp, i32, i64, vp]),
        'midas_merge_tables_fetch': (i32, [vp, vp, i32, i64, vp]),
        'midas_snps_tableset_read_counts_device': (i32, [vp, vp, i64, i64, i32, vp, vp, vp, C.c_char_p]),
        'midas_snps_parse_rows_device': (i32, [vp, vp, i64, i32, vp, i64, C.POINTER(i64), C.POINTER(i64)]),
        'midas_merge_sites_resident': (i32, [vp, C.POINTER(MergeParams), vp, i64, vp] + [vp] * 5 + [C.POINTER(C.c_float)]),
        'midas_merge_sites_tables_resident': (i32, [vp, C.POINTER(MergeParams), vp, i64, vp, C.c_char_p, C.c_char_p, C.c_char_p, i64,
                                                    vp, vp, vp, C.POINTER(i64), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
        'midas_snps_table_open': (i32, [C.c_char_p, i64, i32, C.POINTER(vp), C.c_char_p]),
        'midas_snps_table_close': (None, [vp]),
        'midas_snps_table_rows': (i64, [vp]),
        'midas_snps_table_key_bytes': (i64, [vp]),
        'midas_snps_table_copy': (i32, [vp, vp, vp, vp]),
        'midas_genes_count': (i32, [vp, C.POINTER(Thresholds), C.POINTER(_Reads), vp, i64, vp, vp, vp, vp, C.POINTER(C.c_float)]),
        'midas_genes_terms': (i32, [vp, C.POINTER(Thresholds), C.POINTER(_Reads), vp, i64, vp, vp, C.POINTER(C.c_float)]),
        'midas_genes_count_device': (i32, [vp, C.POINTER(Thresholds), C.POINTER(_Reads), vp, i64, vp, vp, vp, vp, C.POINTER(C.c_float)]),
        'midas_genes_count_timing': (i32, [vp, vp]),
        'midas_genes_count_bam': (i32, [vp, vp, C.POINTER(Thresholds), i64, vp, vp, vp, vp, vp, vp, C.c_char_p]),
        'midas_genes_sum': (i32, [vp, i64, vp, vp, i64, vp, vp, vp, C.POINTER(C.c_float)]),
        'midas_merge_sites': (i32, [vp, C.POINTER(MergeParams), i32, i64, C.POINTER(vp), vp] + [vp] * 5 + [C.POINTER(C.c_float)]),
        'midas_bam_open_share': (i32, [C.c_char_p, i32, i32, i64, C.POINTER(vp), vp, C.c_char_p]),
        'midas_comm_device_key': (i32, [vp, C.c_char_p]),
        'midas_comm_unique_id': (i32, [vp, C.c_char_p]),
        'midas_comm_probe': (i32, [C.POINTER(i32), C.c_char_p]),
        'midas_comm_create': (i32, [vp, vp, i32, i32, C.POINTER(vp), C.c_char_p]),
        'midas_comm_destroy': (None, [vp]),
        'midas_comm_all_gather': (i32, [vp, vp, vp, i64, C.c_char_p]),
        'midas_comm_all_to_all_v': (i32, [vp, vp, vp, vp, vp, C.c_char_p]),
        'midas_genes_merge_map_open': (i32, [C.c_char_p, C.c_char_p, C.POINTER(vp), C.c_char_p]),
        'midas_genes_merge_map_n_clusters': (i64, [vp]),
        'midas_genes_merge_map_n_genes': (i64, [vp]),
        'midas_genes_merge_map_columns': (i32, [vp, vp, vp]),
        'midas_genes_merge_map_close': (None, [vp]),
        'midas_genes_merge_tables_open': (i32, [i32, vp, i32, C.POINTER(vp), C.c_char_p]),
        'midas_genes_merge_tables_rows': (i64, [vp, i32]),
        'midas_genes_merge_tables_resolve': (i32, [vp, vp, i32, i32, C.c_char_p]),
        'midas_genes_merge_tables_columns': (i32, [vp, i32, vp, C.POINTER(i64), C.POINTER(i32)]),
        'midas_genes_merge_tables_close': (None, [vp]),
        'midas_genes_merge': (i32, [vp, i32, vp, vp, vp, vp, vp, i64, C.c_double, i32, i64, C.POINTER(i64)] + [vp] * 5
                              + [C.POINTER(C.c_float)]),
        'midas_genes_merge_write_matrix': (i32, [C.c_char_p, C.c_char_p, i32, i64, vp, vp, vp, i32, vp, vp, i32, C.c_char_p]),
        'midas_genes_merge_format_f64': (i32, [i64, vp, vp, i64, C.POINTER(i64)]),
        'midas_sites_tables_open': (i32, [C.c_char_p, C.POINTER(vp), C.c_char_p]),
        'midas_sites_tables_counts': (i32, [vp, vp]),
        'midas_sites_tables_columns': (i32, [vp, vp, vp]),
        'midas_sites_tables_close': (None, [vp]),
        'midas_sites_tables_positions': (i32, [vp, vp, vp, C.c_char_p]),
        'midas_sites_ld': (i32, [vp, vp, i64, vp, i64, i64, vp, i32] + [vp] * 6 + [i64, i64] + [vp] * 7),
        'midas_sites_parse_cell': (i32, [i32, C.c_char_p, i64, vp]),
        'midas_sites_scan': (i32, [vp, vp, i64, vp, i64, i64, vp, vp, vp, vp, i32] + [vp] * 15),
        'midas_sites_scan_resampled': (i32, [vp, vp, i64, vp, i64, i64, vp, vp, vp, vp, i32] + [vp] * 15 + [i64, i32, vp, i32, vp, vp, vp]),
        'midas_sites_scan_classes': (i32, [vp, vp, i64, vp, i64, i64, vp, vp, vp, vp, i32] + [vp] * 15 + [vp, i32]),
        'midas_snps_mt19937_stream': (i32, [vp, vp, i32, i64, i64, i64, vp, vp, vp, vp, vp]),
        'midas_sites_id_markers': (i32, [vp, vp, i64, vp, i64, i64, i64, vp, vp, i32] + [vp] * 6),
        'midas_sites_track_markers': (i32, [vp, vp, i64, vp, i64, i64, i64, vp, i32] + [vp] * 6),
        'midas_sites_consensus_pairs': (i32, [vp, vp, i64, vp, i64, i64, vp, i32] + [vp] * 8),
        'midas_nj_tree': (i32, [vp, i32] + [vp] * 7),
        'midas_sites_pair_diversity': (i32, [vp, vp, i64, vp, i64, i64, vp, i32] + [vp] * 13),
        'midas_sites_write_markers': (i32, [C.c_char_p, vp, i64, vp, C.c_char_p]),
        'midas_sites_write_pairs': (i32, [C.c_char_p, vp, i32, vp, vp, C.c_char_p]),
        'midas_genes_matrix_open': (i32, [C.c_char_p, C.POINTER(vp), C.c_char_p]),
        'midas_genes_matrix_counts': (i32, [vp, vp]),
        'midas_genes_matrix_columns': (i32, [vp, vp, C.POINTER(i64)]),
        'midas_genes_matrix_close': (None, [vp]),
        'midas_genes_compare_parse_cell': (i32, [C.c_char_p, i64, C.POINTER(C.c_double), C.POINTER(i32)]),
        'midas_genes_compare': (i32, [vp, vp, i64, i64, i32, i32, i32, i32, C.c_double] + [vp] * 9),
        'midas_genes_compare_write_pairs': (i32, [C.c_char_p, vp, i32, i32, i32, i64, vp, vp, vp, vp, C.c_char_p]),
        'midas_genes_linkage': (i32, [vp, vp, i64, i64, i32, i32, C.c_double, vp, vp, i64] + [vp] * 8),
        'midas_genes_linkage_write_pairs': (i32, [C.c_char_p, vp, i64, vp, vp, i64, vp, vp, vp, C.c_char_p]),
        'midas_genes_linkage_write_groups': (i32, [C.c_char_p, vp, i64, vp, vp, vp, i64, C.POINTER(i64), C.c_char_p]),
        'midas_genes_assoc': (i32, [vp, vp, i64, i64, i32, i32, vp, vp, vp, i64, C.c_double] + [vp] * 10),
        'midas_genes_assoc_write': (i32, [C.c_char_p, vp, i64] + [vp] * 6 + [i64, vp, vp, vp, C.c_char_p]),
        'midas_species_classify': (i32, [vp, vp, i64, i32, vp, vp, vp, vp, i32, i32, vp, C.c_double, vp, vp, vp, vp, vp, C.POINTER(vp)]),
        'midas_species_result_columns': (i32, [vp, vp, vp, vp]),
        'midas_species_result_lines': (i32, [vp] * 8),
        'midas_species_result_close': (None, [vp]),
        'midas_species_assign': (i32, [i64, vp, vp, vp, i32, vp, i32, vp, i32, vp, vp, vp]),
        'midas_species_parse_number': (i32, [i32, C.c_char_p, i64, vp, C.POINTER(i32)]),
        'midas_species_merge': (i32, [vp, i32, vp, i32, vp, vp, C.c_double, vp, vp, vp, C.POINTER(vp)]),
        'midas_species_merge_result_matrices': (i32, [vp, vp, vp, vp]),
        'midas_species_merge_result_stats': (i32, [vp, vp, vp, vp]),
        'midas_species_merge_result_write': (i32, [vp, C.c_char_p, C.c_char_p, i32, C.c_char_p]),
        'midas_species_merge_result_close': (None, [vp]),
    })
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)          # AttributeError if the symbol is missing: fail loudly
        fn.restype = res
        fn.argtypes = args
    if lib.midas_snps_abi_version() != ABI_VERSION:
        raise MidasSnpsError(ERR_INVALID_ARG, "ABI version mismatch: library %d, binding %d"
                             % (lib.midas_snps_abi_version(), ABI_VERSION))
    _lib = lib
    return lib


EXPORTED_SYMBOLS = [
    'midas_snps_abi_version', 'midas_snps_cpu_budget', 'midas_snps_status_string', 'midas_snps_create', 'midas_snps_destroy',
    'midas_snps_last_error', 'midas_snps_last_error_read', 'midas_snps_set_stream', 'midas_snps_device_info',
    'midas_snps_host_alloc', 'midas_snps_host_free',
    'midas_snps_pileup', 'midas_snps_batch_create', 'midas_snps_batch_destroy', 'midas_snps_batch_run',
    'midas_snps_batch_sync', 'midas_snps_batch_fetch', 'midas_snps_batch_get_info',
    'midas_snps_batch_enable_timing', 'midas_snps_batch_timing', 'midas_snps_batch_time_pileup_only',
    'midas_snps_batch_stats_to_device', 'midas_snps_batch_pack', 'midas_snps_batch_fetch_packed',
    'midas_snps_batch_select_path', 'midas_snps_set_default_path', 'midas_snps_copy_rate', 'midas_snps_stream_rates', 'midas_snps_calibration_pass', 'midas_snps_set_pad_rule', 'midas_snps_set_row_coder',
    'midas_snps_row_coder_counts', 'midas_snps_rows_code', 'midas_snps_scan_u32', 'midas_snps_sort_pairs', 'midas_snps_mt19937_stream',
    'midas_snps_batch_pack_timing', 'midas_snps_batch_fetch_index',
    'midas_bam_open', 'midas_bam_close', 'midas_bam_write', 'midas_bam_n_refs', 'midas_bam_ref', 'midas_bam_load', 'midas_bam_copy', 'midas_bam_columns',
    'midas_bam_open_slice', 'midas_bam_slice_facts', 'midas_bam_slice_marks', 'midas_bam_load_ranges',
    'midas_bam_open_device', 'midas_bam_open_slice_device', 'midas_bam_load_ranges_device', 'midas_snps_inflate_blocks', 'midas_bam_load_device',
    'midas_bam_payload_on_device', 'midas_snps_copy_from_device', 'midas_bam_release_file',
    'midas_bam_load_resident', 'midas_bam_load_ranges_resident', 'midas_bam_is_resident', 'midas_bam_resident_to_columns',
    'midas_snps_batch_create_resident', 'midas_bam_open_share_local', 'midas_bam_share_locate',
    'midas_snps_write_rows', 'midas_snps_write_table', 'midas_snps_write_part', 'midas_snps_write_pieces', 'midas_snps_deflate_rows',
    'midas_snps_tableset_open', 'midas_snps_tableset_read_counts', 'midas_snps_tableset_close', 'midas_snps_batch_write_part',
    'midas_fasta_load', 'midas_fasta_n_records', 'midas_fasta_columns', 'midas_fasta_close',
    'midas_snps_table_open', 'midas_snps_table_open_range', 'midas_snps_table_count_rows', 'midas_snps_table_close', 'midas_snps_table_rows', 'midas_snps_table_key_bytes',
    'midas_snps_table_copy', 'midas_merge_sites', 'midas_genes_count', 'midas_genes_terms', 'midas_genes_sum', 'midas_merge_write_info',
    'midas_genes_count_device', 'midas_genes_count_timing', 'midas_genes_count_bam',
    'midas_merge_write_matrix', 'midas_merge_write_matrix_device', 'midas_merge_sites_tables',
    'midas_merge_tables_create', 'midas_merge_tables_free', 'midas_merge_tables_shape', 'midas_merge_tables_set_host', 'midas_merge_tables_fetch',
    'midas_snps_tableset_read_counts_device', 'midas_snps_parse_rows_device', 'midas_merge_sites_resident', 'midas_merge_sites_tables_resident',
    'midas_bam_open_share',
    'midas_comm_device_key', 'midas_comm_probe', 'midas_comm_unique_id', 'midas_comm_create', 'midas_comm_destroy', 'midas_comm_all_gather', 'midas_comm_all_to_all_v',
    'midas_genes_merge_map_open', 'midas_genes_merge_map_n_clusters', 'midas_genes_merge_map_n_genes', 'midas_genes_merge_map_columns',
    'midas_genes_merge_map_close', 'midas_genes_merge_tables_open', 'midas_genes_merge_tables_rows', 'midas_genes_merge_tables_resolve',
    'midas_genes_merge_tables_columns', 'midas_genes_merge_tables_close', 'midas_genes_merge', 'midas_genes_merge_write_matrix',
    'midas_genes_merge_format_f64',
    'midas_genes_matrix_open', 'midas_genes_matrix_counts', 'midas_genes_matrix_columns', 'midas_genes_matrix_close',
    'midas_genes_compare_parse_cell', 'midas_genes_compare', 'midas_genes_compare_write_pairs',
    'midas_genes_linkage', 'midas_genes_linkage_write_pairs', 'midas_genes_linkage_write_groups',
    'midas_genes_assoc', 'midas_genes_assoc_write',
]
# the analysis entry points (snp_diversity.py, call_consensus.py, strain_tracking.py): bound above like the rest, listed by themselves
SITES_SYMBOLS = ['midas_sites_tables_open', 'midas_sites_tables_counts', 'midas_sites_tables_columns', 'midas_sites_tables_close',
                 'midas_sites_parse_cell', 'midas_sites_scan', 'midas_sites_scan_resampled', 'midas_sites_scan_classes', 'midas_sites_id_markers', 'midas_sites_track_markers',
                 'midas_sites_write_markers', 'midas_sites_write_pairs', 'midas_sites_consensus_pairs', 'midas_sites_pair_diversity',
                 'midas_sites_tables_positions', 'midas_sites_ld']
# snp_trees.py (neighbour joining over the consensus distances): bound above like the rest, listed by itself
TREE_SYMBOLS = ['midas_nj_tree']


# run_species.py (the m8 classify step and the serial assignment): bound above like the rest, listed by themselves
SPECIES_SYMBOLS = ['midas_species_classify', 'midas_species_result_columns', 'midas_species_result_lines', 'midas_species_result_close',
                   'midas_species_assign', 'midas_species_parse_number']
SPECIES_PHASES = ('upload', 'line index', 'fields', 'lookup', 'filter + sort + group', 'best hits', 'download')
SPECIES_REASONS = {1: 'fields', 2: 'target', 3: 'qlen', 4: 'aln', 5: 'number', 6: 'cutoff', 7: 'score nan'}
# merge_species.py (the species profiles merged): bound above like the rest, listed by themselves
SPECIES_MERGE_SYMBOLS = ['midas_species_merge', 'midas_species_merge_result_matrices', 'midas_species_merge_result_stats',
                         'midas_species_merge_result_write', 'midas_species_merge_result_close']
SPECIES_MERGE_PHASES = ('read (wait)', 'upload', 'index', 'fields', 'lookup + scatter', 'statistics', 'download')
SPECIES_MERGE_REASONS = {1: 'header species_id', 2: 'header count_reads', 3: 'header coverage', 4: 'header relative_abundance', 5: 'unknown species',
                         6: 'species twice', 7: 'cell count_reads', 8: 'cell coverage', 9: 'cell relative_abundance', 10: 'non-finite coverage',
                         11: 'non-finite relative_abundance', 12: 'count_reads range', 13: 'species missing'}
SPECIES_MERGE_STATS = ('mean_coverage', 'median_coverage', 'mean_abundance', 'median_abundance')


def species_parse_number(text: bytes, kind: str = 'float'):
    """float() / int() of an m8 field as the classify step takes it (midas_species_parse_number) -> (value, decoded by the
    device's own decoder), or None when it is no number."""
    lib = load_library()
    fast = C.c_int32(0)
    out = C.c_double(0) if kind == 'float' else C.c_int64(0)
    if lib.midas_species_parse_number(0 if kind == 'float' else 1, text, len(text), C.byref(out), C.byref(fast)) != 0:
        return None
    return out.value, bool(fast.value)


def mt_states(py_state=None, np_state=None):
    """(624 words, position) of Python's and numpy's global generators, or of the given random.getstate() /
    np.random.get_state() values."""
    import random
    ps = py_state if py_state is not None else random.getstate()
    ns = np_state if np_state is not None else np.random.get_state()
    return (np.array(ps[1][:624], np.uint32), int(ps[1][624])), (np.ascontiguousarray(ns[1], np.uint32), int(ns[2]))


def species_assign(indptr, hit_species, hit_aln, reads, aln, py_state=None, np_state=None):
    """midas_species_assign(): the ambiguous reads of Context.species_classify given out in order, starting from the per-species
    `reads` and `aln` sums of the unique reads -> (reads, aln, (words drawn from Python's generator, doubles from numpy's)).
    Needs no device.  The generators' states are read, not advanced."""
    lib = load_library()
    (pw, pp), (nw, npos) = mt_states(py_state, np_state)
    ip = np.ascontiguousarray(indptr, np.int64)
    hs, ha = np.ascontiguousarray(hit_species, np.int32), np.ascontiguousarray(hit_aln, np.int32)
    r, a = np.array(reads, np.int64), np.array(aln, np.int64)
    draws = np.zeros(2, np.int64)
    p = lambda x: x.ctypes.data_as(C.c_void_p) if x.size else None
    st = lib.midas_species_assign(ip.size - 1, p(ip), p(hs), p(ha), r.size, p(pw), pp, p(nw), npos, p(r), p(a), p(draws))
    if st != 0:
        raise MidasSnpsError(st, "midas_species_assign: " + lib.midas_snps_status_string(st).decode())
    return r, a, (int(draws[0]), int(draws[1]))


# the SAM decode (run_midas.py snps --sam, genes --sam): bound above like the rest, listed by themselves
SAM_SYMBOLS = ['midas_sam_load_device', 'midas_sam_decode_timing', 'midas_sam_load_device_order', 'midas_sam_load_resident']
SAM_ORDERS = {'coordinate': 0, 'file': 1}        # MIDAS_SAM_ORDER_*
GENES_BAM_PHASES = ('upload', 'inflate + crc', 'walk + stitch + offsets', 'facts kernel', 'filter + sort + sums', 'download')
GENES_BAM_STATS = ('records', 'dropped', 'blocks', 'inflated_bytes', 'chunks', 'chunks_again')
SAM_PHASES = ('map + header', 'upload', 'line index', 'pass 1 (fields)', 'scans', 'pass 2 (payload)', 'sort + gather', 'columns down')


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
    err = C.create_string_buffer(256)
    st = lib.midas_snps_write_rows(path.encode(), 1 if append else 0, ref_id.encode(), allele.shape[0],
                                   allele.ctypes.data_as(C.c_void_p), counts.ctypes.data_as(C.c_void_p),
                                   int(gz_level), int(threads), err)
    if st != 0:
        raise MidasSnpsError(st, err.value.decode())


ROWS_PER_MEMBER = 16384     # MIDAS_SNPS_ROWS_PER_MEMBER: pieces of a contig start at multiples of this


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
    err = C.create_string_buffer(256)
    if first_pos is not None:
        fp = (C.c_int64 * max(n, 1))(*[int(x) for x in first_pos])
        st = lib.midas_snps_write_pieces(path.encode(), 1 if (header is None or header) else 0, n, ids, ns, fp, pa, pc,
                                         int(gz_level), int(threads), err)
    elif header is None:
        st = lib.midas_snps_write_table(path.encode(), n, ids, ns, pa, pc, int(gz_level), int(threads), err)
    else:
        st = lib.midas_snps_write_part(path.encode(), 1 if header else 0, n, ids, ns, pa, pc, int(gz_level), int(threads), err)
    if st != 0:
        raise MidasSnpsError(st, err.value.decode())


class _Genes(C.Structure):
    _fields_ = [("n_genes", C.c_int64), ("scaffold_id", C.c_void_p), ("start", C.c_void_p), ("end", C.c_void_p),
                ("strand", C.c_char_p), ("gene_type", C.c_void_p), ("gene_id", C.c_void_p), ("seq", C.c_void_p)]


def write_merge_info(path: str, header_line: str, keep: np.ndarray, keys, key_off: np.ndarray, res: dict, genes: list,
                     threads: int = 0, site_id_base: int = 0):
    """snps_info.txt for the kept sites (midas_merge_write_info): annotation + the per-site calls.  keys / key_off as
    returned by read_snps_table, res = Context.merge_sites(...), genes = the species' genes in the reference's order
    (dicts with scaffold_id, start, end, strand, gene_type, gene_id, seq)."""
    lib = load_library()
    keep = np.ascontiguousarray(keep, dtype=np.int64)
    key_off = np.ascontiguousarray(key_off, dtype=np.int64)
    kb = np.frombuffer(keys, dtype=np.uint8) if not isinstance(keys, np.ndarray) else keys
    calls = res['major'].base if res['major'].base is not None else np.stack([res['major'], res['minor'], res['snp_type'], res['flag']], 1)
    calls = np.ascontiguousarray(calls, dtype=np.uint8)
    cs = np.ascontiguousarray(res['count_samples'], dtype=np.uint32)
    pooled = np.ascontiguousarray(res['pooled'], dtype=np.uint64)
    n = len(genes)

    def strs(field):
        vals = [str(g[field]).encode() for g in genes]
        return (C.c_char_p * max(n, 1))(*vals)
    sid, gty, gid, seq = strs('scaffold_id'), strs('gene_type'), strs('gene_id'), strs('seq')
    start = np.array([g['start'] for g in genes], dtype=np.int64)
    end = np.array([g['end'] for g in genes], dtype=np.int64)
    strand = "".join(str(g['strand'])[:1] or '+' for g in genes).encode()
    gs = _Genes(n, C.cast(sid, C.c_void_p), start.ctypes.data_as(C.c_void_p), end.ctypes.data_as(C.c_void_p), strand,
                C.cast(gty, C.c_void_p), C.cast(gid, C.c_void_p), C.cast(seq, C.c_void_p))
    err = C.create_string_buffer(256)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    st = lib.midas_merge_write_info(path.encode(), header_line.encode(), keep.shape[0], p(keep), p(kb), p(key_off), p(calls),
                                    p(cs), p(pooled), C.byref(gs), int(threads), int(site_id_base), err)
    if st != 0:
        raise MidasSnpsError(st, err.value.decode())


def write_merge_matrix(path: str, header_line: str, keep: np.ndarray, depth: np.ndarray, minor_count=None, threads: int = 0,
                       site_id_base: int = 0):
    """snps_depth.txt (minor_count None) / snps_freq.txt of merge_midas.py snps for the kept sites (midas_merge_write_matrix).
    depth, minor_count: [n_samples, n_sites] uint32 as returned by Context.merge_sites."""
    lib = load_library()
    keep = np.ascontiguousarray(keep, dtype=np.int64)
    depth = np.ascontiguousarray(depth, dtype=np.uint32)
    S, n = depth.shape
    mc = None
    if minor_count is not None:
        mc = np.ascontiguousarray(minor_count, dtype=np.uint32)
        assert mc.shape == depth.shape
    err = C.create_string_buffer(256)
    st = lib.midas_merge_write_matrix(path.encode(), header_line.encode(), keep.shape[0], keep.ctypes.data_as(C.c_void_p),
                                      S, n, depth.ctypes.data_as(C.c_void_p),
                                      mc.ctypes.data_as(C.c_void_p) if mc is not None else None, int(threads), int(site_id_base), err)
    if st != 0:
        raise MidasSnpsError(st, err.value.decode())


def write_merge_matrix_device(ctx, path: str, header_line: str, keep: np.ndarray, depth: np.ndarray, minor_count=None,
                              site_id_base: int = 0) -> float:
    """write_merge_matrix with the rows formatted on ctx's device (midas_merge_write_matrix_device): the same file, byte for
    byte.  Stricter than the host writer where the device needs it (MidasSnpsError): every keep[r] in [0, n_sites),
    site_id_base >= 0, no minor count above its non-zero depth, kept rows ascending unless the arrays fit one upload chunk
    (none of which merge_sites' outputs can violate).  -> device time of the formatter, ms."""
    keep = np.ascontiguousarray(keep, dtype=np.int64)
    depth = np.ascontiguousarray(depth, dtype=np.uint32)
    S, n = depth.shape
    mc = None
    if minor_count is not None:
        mc = np.ascontiguousarray(minor_count, dtype=np.uint32)
        assert mc.shape == depth.shape
    ms = C.c_float(0)
    st = ctx._lib.midas_merge_write_matrix_device(ctx._h, path.encode(), header_line.encode(), keep.shape[0],
                                                  keep.ctypes.data_as(C.c_void_p), S, n, depth.ctypes.data_as(C.c_void_p),
                                                  mc.ctypes.data_as(C.c_void_p) if mc is not None else None, int(site_id_base),
                                                  C.byref(ms))
    ctx._check(st)
    return float(ms.value)


def count_snps_rows(path: str) -> int:
    """Rows of a <species>.snps.gz without inflating it, or -1 when the file does not say (midas_snps_table_count_rows)."""
    lib = load_library()
    n = C.c_int64(-1)
    err = C.create_string_buffer(256)
    st = lib.midas_snps_table_count_rows(path.encode(), C.byref(n), err)
    if st != 0:
        raise MidasSnpsError(st, err.value.decode())
    return int(n.value)


def read_snps_table(path: str, max_rows: int = -1, want_keys: bool = True, row_begin: int = 0):
    """Parse one <species>.snps.gz with the native reader -> (counts[n,4] u32, keys | None, key_off | None);
    keys is a byte buffer, row i's 'ref_id|ref_pos|ref_allele' is bytes(keys[key_off[i]:key_off[i + 1]]).
    Rows [row_begin, max_rows) of the table (max_rows < 0: to the end)."""
    lib = load_library()
    h = C.c_void_p()
    err = C.create_string_buffer(256)
    st = lib.midas_snps_table_open_range(path.encode(), int(row_begin), int(max_rows), 1 if want_keys else 0, C.byref(h), err)
    if st != 0:
        raise MidasSnpsError(st, err.value.decode())
    try:
        n = int(lib.midas_snps_table_rows(h))
        counts = np.empty((n, 4), np.uint32)
        keys = np.empty(int(lib.midas_snps_table_key_bytes(h)), np.uint8) if want_keys else None
        key_off = np.empty(n + 1, np.int64) if want_keys else None
        p = lambda x: x.ctypes.data_as(C.c_void_p) if x is not None else None
        lib.midas_snps_table_copy(h, p(counts), p(keys), p(key_off))
    finally:
        lib.midas_snps_table_close(h)
    return counts, (memoryview(keys) if want_keys else None), key_off


def read_snps_counts(paths, row_begin: int = 0, max_rows: int = -1):
    """The count columns of several samples' <species>.snps.gz in one parallel region (midas_snps_tableset_*):
    -> list of counts[n,4] u32, one per path, n = rows [row_begin, max_rows) of the SHORTEST table (max_rows < 0: its
    end) -- the reference's zip over the samples' files stops there too.  None when one of the files does not announce
    its rows (written by the reference): read those with read_snps_table."""
    lib = load_library()
    n = len(paths)
    arr = (C.c_char_p * n)(*[p.encode() for p in paths])
    rows = np.empty(n, np.int64)
    h = C.c_void_p()
    err = C.create_string_buffer(256)
    st = lib.midas_snps_tableset_open(n, arr, C.byref(h), rows.ctypes.data_as(C.c_void_p), err)
    if st != 0:
        raise MidasSnpsError(st, err.value.decode())
    try:
        if (rows < 0).any():
            return None
        hi = int(rows.min()) if max_rows < 0 else min(int(rows.min()), int(max_rows))
        m = max(0, hi - int(row_begin))
        out = [np.empty((m, 4), np.uint32) for _ in range(n)]
        ptrs = (C.c_void_p * n)(*[a.ctypes.data for a in out])
        st = lib.midas_snps_tableset_read_counts(h, int(row_begin), m, ptrs, err)
        if st != 0:
            raise MidasSnpsError(st, err.value.decode())
        return out
    finally:
        lib.midas_snps_tableset_close(h)


def read_bam(path: str, ctx=None, payload_on_device: bool = False, resident: bool = False):
    """Decode a BAM with the native reader -> (ref_names, ref_lengths, refid[int32], ReadsSoA).  The arrays are views of
    the decoder's own buffers (no copy); the native handle lives as long as any of them does.  ctx (a Context): the BGZF
    blocks are inflated on its device instead of by the host's threads (midas_bam_open_device); with payload_on_device SEQ,
    QUAL and CIGAR are also cut out of the inflated stream there and never come down (midas_bam_load_device): the ReadsSoA
    carries their device addresses (`device`) and only that context's batches can take it."""
    lib = load_library()
    h = C.c_void_p()
    err = C.create_string_buffer(256)
    if resident:
        # ONE pass from the BAM's bytes to the kernel's input: every column stays on the device, in the direct layout; refID
        # alone comes down (midas_bam_load_resident).  More payload than the layout addresses: the columns' way.
        if ctx is None or not getattr(ctx, 'inflates', False):
            raise MidasSnpsError(ERR_INVALID_ARG, "resident needs a device context")
        n, total = C.c_int64(), C.c_int64()
        st = lib.midas_bam_load_resident(path.encode(), ctx._h, C.byref(h), C.byref(n), C.byref(total), err)
        if st == ERR_UNSUPPORTED:
            return read_bam(path, ctx, payload_on_device=True)
        if st != 0:
            raise MidasSnpsError(st, err.value.decode())
        owner = _BamOwner(lib, h)
        names, lens = _bam_refs(lib, h)
        ptrs = (C.c_void_p * 12)()
        lib.midas_bam_columns(h, ptrs)
        refid = np.asarray(_Column(owner, ptrs[0] or 0, int(n.value), np.int32))
        return names, lens, refid, ResidentReads(lib, h, owner, int(n.value), int(total.value))
    if payload_on_device:
        if ctx is None or not getattr(ctx, 'inflates', False):
            raise MidasSnpsError(ERR_INVALID_ARG, "payload_on_device needs a device context")
        n, sb, qb, nc = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        st = lib.midas_bam_load_device(path.encode(), ctx._h, C.byref(h), C.byref(n), C.byref(sb), C.byref(qb), C.byref(nc), err)
        if st != 0:
            raise MidasSnpsError(st, err.value.decode())
        owner = _BamOwner(lib, h)
        names, lens = _bam_refs(lib, h)
        refid, reads = _bam_columns(lib, h, int(n.value), int(sb.value), int(qb.value), int(nc.value), owner, on_device=True)
        return names, lens, refid, reads
    if ctx is not None and getattr(ctx, 'inflates', False):
        st = lib.midas_bam_open_device(path.encode(), ctx._h, C.byref(h), err)
    else:
        st = lib.midas_bam_open(path.encode(), C.byref(h), err)
    if st != 0:
        raise MidasSnpsError(st, err.value.decode())
    owner = _BamOwner(lib, h)
    names, lens = _bam_refs(lib, h)
    n, sb, qb, nc = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
    st = lib.midas_bam_load(h, C.byref(n), C.byref(sb), C.byref(qb), C.byref(nc), err)
    if st != 0:
        raise MidasSnpsError(st, err.value.decode())
    refid, reads = _bam_columns(lib, h, int(n.value), int(sb.value), int(qb.value), int(nc.value), owner)
    return names, lens, refid, reads


TABLES_READ_PHASES = ('upload', 'inflate + crc', 'index', 'parse')
TABLES_READ_STATS = ('tables', 'members', 'groups', 'compressed_bytes', 'inflated_bytes', 'rows', 'groups_decoded_twice')


class MergeTables:
    """The samples' count tables of one merge, resident on the device (midas_merge_tables_*): n_samples x n_rows x 4 u32.  Owns
    the set and frees it (close, `with`, or when collected).  n_sites: the rows a merge takes (<= n_rows; the caller lowers it
    when a table it read by itself turned out shorter).  stats / ms: what the device readers reported (read_snps_counts_device)."""

    def __init__(self, ctx: "Context", n_samples: int, n_rows: int):
        self._ctx, self._lib = ctx, ctx._lib
        h = C.c_void_p()
        ctx._check(self._lib.midas_merge_tables_create(ctx._h, int(n_samples), int(n_rows), C.byref(h)))
        self._h = h
        self.n_samples, self.n_rows, self.n_sites = int(n_samples), int(n_rows), int(n_rows)
        self.stats, self.ms = {}, {}

    def set_host(self, sample: int, counts):
        """The first len(counts) rows of sample `sample` from a host array [n, 4] u32."""
        a = np.ascontiguousarray(counts, dtype=np.uint32)
        assert a.ndim == 2 and a.shape[1] == 4 and a.shape[0] <= self.n_rows
        self._ctx._check(self._lib.midas_merge_tables_set_host(self._ctx._h, self._h, int(sample), a.shape[0], a.ctypes.data_as(C.c_void_p)))

    def fetch(self, sample: int, n_rows: int = None):
        n = self.n_sites if n_rows is None else int(n_rows)
        out = np.empty((n, 4), np.uint32)
        self._ctx._check(self._lib.midas_merge_tables_fetch(self._ctx._h, self._h, int(sample), n, out.ctypes.data_as(C.c_void_p)))
        return out

    def close(self):
        if getattr(self, '_h', None):
            self._lib.midas_merge_tables_free(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


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
    if ctx is None or not getattr(ctx, 'inflates', False):
        raise MidasSnpsError(ERR_INVALID_ARG, "open_bam_device needs a device context")
    lib = load_library()
    h = C.c_void_p()
    err = C.create_string_buffer(256)
    out3 = (C.c_int64 * 3)()
    st = lib.midas_bam_open_share(path.encode(), 0, 1, 0, C.byref(h), out3, err)
    if st != 0:
        raise MidasSnpsError(st, err.value.decode())
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
    if ctx is None or not getattr(ctx, 'inflates', False):
        raise MidasSnpsError(ERR_INVALID_ARG, "read_sam needs a device context (the SAM text is parsed and sorted on the GPU)")
    if order not in SAM_ORDERS:
        raise MidasSnpsError(ERR_INVALID_ARG, "read_sam: order is 'coordinate' or 'file', not %r" % (order,))
    if resident and order != 'coordinate':
        raise MidasSnpsError(ERR_INVALID_ARG, "read_sam: resident records are coordinate-sorted, order=%r is not for them" % (order,))
    lib = load_library()
    h = C.c_void_p()
    err = C.create_string_buffer(256)
    if resident:
        n, total = C.c_int64(), C.c_int64()
        st = lib.midas_sam_load_resident(path.encode(), ctx._h, C.byref(h), C.byref(n), C.byref(total), err)
        if st == ERR_UNSUPPORTED:
            return read_sam(path, ctx, order)
        if st != 0:
            raise MidasSnpsError(st, err.value.decode())
        owner = _BamOwner(lib, h)
        names, lens = _bam_refs(lib, h)
        ptrs = (C.c_void_p * 12)()
        lib.midas_bam_columns(h, ptrs)
        refid = np.asarray(_Column(owner, ptrs[0] or 0, int(n.value), np.int32))
        return names, lens, refid, ResidentReads(lib, h, owner, int(n.value), int(total.value))
    n, sb, qb, nc = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
    if order == 'coordinate':
        st = lib.midas_sam_load_device(path.encode(), ctx._h, C.byref(h), C.byref(n), C.byref(sb), C.byref(qb), C.byref(nc), err)
    else:
        st = lib.midas_sam_load_device_order(path.encode(), ctx._h, SAM_ORDERS[order], C.byref(h), C.byref(n), C.byref(sb), C.byref(qb),
                                             C.byref(nc), err)
    if st != 0:
        raise MidasSnpsError(st, err.value.decode())
    owner = _BamOwner(lib, h)
    names, lens = _bam_refs(lib, h)
    refid, reads = _bam_columns(lib, h, int(n.value), int(sb.value), int(qb.value), int(nc.value), owner, on_device=True)
    return names, lens, refid, reads


def sam_decode_timing(ctx) -> dict:
    """Host-clock milliseconds of the phases of the context's last read_sam (midas_sam_decode_timing), by name."""
    ms = (C.c_float * 8)()
    st = load_library().midas_sam_decode_timing(ctx._h, ms)
    if st != 0:
        raise MidasSnpsError(st, "midas_sam_decode_timing failed")
    return dict(zip(SAM_PHASES, (float(x) for x in ms)))


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


class _Column:
    def __init__(self, owner, ptr, n, dtype):
        self._owner = owner
        dt = np.dtype(dtype)
        self.__array_interface__ = {'shape': (int(n),), 'typestr': dt.str, 'data': (int(ptr) if n else 0, True), 'version': 3} \
            if n else np.empty(0, dt).__array_interface__


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
    err = C.create_string_buffer(256)
    st = lib.midas_fasta_load(n, c_paths, int(threads), C.byref(h), err)
    if st != 0:
        raise MidasSnpsError(st, err.value.decode() or "midas_fasta_load failed")
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


class _GenesOwner:
    def __init__(self, lib, h, close):
        self._lib, self._h, self._close = lib, h, close

    def __del__(self):
        if self._h:
            getattr(self._lib, self._close)(self._h)
            self._h = None


class GeneClusterMap:
    """read_cluster_map (midas/merge/genes.py:91-98) read natively (midas_genes_merge_map_*): gene_info.txt[.gz] ->
    centroid_99 -> `cluster_column`.  .cluster_ids / .cluster_off: the distinct clusters in sorted byte order (index = output
    row order); .gene_ids / .gene_off / .gene_cluster: the distinct centroid_99 ids in first-appearance order and their
    clusters.  Read-only views owned by the handle."""

    def __init__(self, path: str, cluster_column: str):
        lib = load_library()
        h = C.c_void_p()
        err = C.create_string_buffer(1024)
        st = lib.midas_genes_merge_map_open(path.encode(), cluster_column.encode(), C.byref(h), err)
        if st != 0:
            raise MidasSnpsError(st, err.value.decode(errors='replace') or "midas_genes_merge_map_open failed")
        self._owner = _GenesOwner(lib, h, 'midas_genes_merge_map_close')
        self.path = path
        self.n_clusters = int(lib.midas_genes_merge_map_n_clusters(h))
        self.n_genes = int(lib.midas_genes_merge_map_n_genes(h))
        ptrs, sizes = (C.c_void_p * 5)(), (C.c_int64 * 2)()
        lib.midas_genes_merge_map_columns(h, ptrs, sizes)
        col = lambda k, n, dt: np.asarray(_Column(self._owner, ptrs[k] or 0, n, dt))
        self.cluster_ids = col(0, int(sizes[0]), np.uint8)
        self.cluster_off = col(1, self.n_clusters + 1, np.int64)
        self.gene_ids = col(2, int(sizes[1]), np.uint8)
        self.gene_off = col(3, self.n_genes + 1, np.int64)
        self.gene_cluster = col(4, self.n_genes, np.uint32)

    @property
    def handle(self):
        return self._owner._h

    def cluster(self, k: int) -> bytes:
        return bytes(self.cluster_ids[int(self.cluster_off[k]):int(self.cluster_off[k + 1])])


class GeneTables:
    """The samples' genes/output/<species>.genes.gz tables read natively, one worker per file (midas_genes_merge_tables_*):
    per sample .ids / .id_off (kept rows' gene ids), .copy / .depth (f64), .reads (i64); after resolve(), .cluster (uint32)
    and .same_as (the earlier sample whose cluster vector it shares, or -1).  Read-only views owned by the handle."""

    def __init__(self, paths, threads: int = 0):
        lib = load_library()
        n = len(paths)
        c_paths = (C.c_char_p * max(n, 1))(*[p.encode() for p in paths])
        h = C.c_void_p()
        err = C.create_string_buffer(1024)
        st = lib.midas_genes_merge_tables_open(n, c_paths, int(threads), C.byref(h), err)
        if st != 0:
            raise MidasSnpsError(st, err.value.decode(errors='replace') or "midas_genes_merge_tables_open failed")
        self._lib = lib
        self._owner = _GenesOwner(lib, h, 'midas_genes_merge_tables_close')
        self.paths = list(paths)
        self.rows = [int(lib.midas_genes_merge_tables_rows(h, k)) for k in range(n)]
        self.resolved = False
        self._columns()

    def _columns(self):
        lib, h = self._lib, self._owner._h
        self.ids, self.id_off, self.copy, self.depth, self.reads, self.cluster, self.same_as = [], [], [], [], [], [], []
        for k, n in enumerate(self.rows):
            ptrs, nb, same = (C.c_void_p * 6)(), C.c_int64(0), C.c_int32(-1)
            lib.midas_genes_merge_tables_columns(h, k, ptrs, C.byref(nb), C.byref(same))
            col = lambda j, m, dt: np.asarray(_Column(self._owner, ptrs[j] or 0, m, dt))
            self.ids.append(col(0, int(nb.value), np.uint8))
            self.id_off.append(col(1, n + 1, np.int64))
            self.copy.append(col(2, n, np.float64))
            self.depth.append(col(3, n, np.float64))
            self.reads.append(col(4, n, np.int64))
            self.cluster.append(col(5, n, np.uint32) if self.resolved else None)
            self.same_as.append(int(same.value))

    def resolve(self, cmap: "GeneClusterMap", reuse: bool = True, threads: int = 0):
        err = C.create_string_buffer(1024)
        st = self._lib.midas_genes_merge_tables_resolve(self._owner._h, cmap.handle, 1 if reuse else 0, int(threads), err)
        if st != 0:
            raise MidasSnpsError(st, err.value.decode(errors='replace') or "midas_genes_merge_tables_resolve failed")
        self.resolved = True
        self._columns()     # (a sample that shares an earlier one's vector views the same memory: one class on the device)


GENES_MATRIX_KINDS = {'presabs': 0, 'copynum': 1, 'depth': 1, 'reads': 2}


def write_genes_matrix(path: str, header_line: str, kind: str, row_cluster, cmap: "GeneClusterMap", values, state, threads: int = 0):
    """genes_<kind>.txt of merge_midas.py genes (midas_genes_merge_write_matrix): row_cluster [R] uint32, values / state
    [R, S] as Context.genes_merge returns them (presabs reads state only)."""
    lib = load_library()
    rc = np.ascontiguousarray(row_cluster, dtype=np.uint32)
    st_ = np.ascontiguousarray(state, dtype=np.uint8)
    k = GENES_MATRIX_KINDS[kind]
    vals = None if k == 0 else np.ascontiguousarray(values, dtype=np.float64 if k == 1 else np.int64)
    R = rc.shape[0]
    S = st_.shape[1] if st_.ndim == 2 else 0
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None
    err = C.create_string_buffer(1024)
    st = lib.midas_genes_merge_write_matrix(path.encode(), header_line.encode(), k, R, p(rc), p(cmap.cluster_ids),
                                            p(cmap.cluster_off), S, p(vals), p(st_), int(threads), err)
    if st != 0:
        raise MidasSnpsError(st, err.value.decode(errors='replace'))


def format_repr_f64(values) -> list:
    """Python's repr() of every double, by the matrix writer's formatter (midas_genes_merge_format_f64)."""
    lib = load_library()
    v = np.ascontiguousarray(values, dtype=np.float64)
    out = np.empty(33 * v.shape[0] + 1, np.uint8)
    n = C.c_int64(0)
    st = lib.midas_genes_merge_format_f64(v.shape[0], v.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), out.shape[0],
                                          C.byref(n))
    if st != 0:
        raise MidasSnpsError(st, "midas_genes_merge_format_f64 failed")
    return out[:n.value].tobytes().decode().split('\n')[:-1]


SITES_WEIGHT, SITES_ROUND, SITES_POOLED, SITES_PER_GENE, SITES_MASK_ONLY, SITES_SEQ, SITES_SUMS = 1, 2, 4, 8, 16, 32, 64
SITES_LD_SAME_GENE = 128     # MIDAS_SITES_LD_SAME_GENE
SITES_LD_MAX_BINS = 4096     # the most distance bins of midas_sites_ld
SITES_MAX_CLASSES = 4        # MIDAS_SITES_MAX_CLASSES
SITES_PAIR_TILE = 64         # MIDAS_SITES_PAIR_TILE: samples a side of the pair kernel's tile
ALLELE_LETTERS = 'ATCG'      # the order of the allele codes and of the count columns of strain_tracking.py id_markers


class SitesTables:
    """One species directory of `merge_midas.py snps` (midas_sites_tables_*): snps_summary.txt and snps_info.txt as columns,
    snps_freq.txt / snps_depth.txt mapped as text.  String columns are (.x_pool uint8, .x_off int64) pairs read through
    .strings(name); .freq_text / .depth_text are the matrices' rows after the header line.  Views owned by the handle."""

    STRING_COLUMNS = ('sample_id', 'site_id', 'ref_allele', 'major_allele', 'minor_allele', 'locus_type', 'site_type', 'gene_id',
                      'matrix_sample_id')

    def __init__(self, indir: str):
        lib = load_library()
        h = C.c_void_p()
        err = C.create_string_buffer(1024)
        st = lib.midas_sites_tables_open(indir.encode(), C.byref(h), err)
        if st != 0:
            raise MidasSnpsError(st, err.value.decode(errors='replace') or "midas_sites_tables_open failed")
        self._owner = _GenesOwner(lib, h, 'midas_sites_tables_close')
        self.dir = indir
        counts = (C.c_int64 * 8)()
        lib.midas_sites_tables_counts(h, counts)
        self.n_samples, self.n_sites, self.n_genes, self.n_columns = (int(counts[k]) for k in range(4))
        self.freq_columns = int(counts[6])
        ptrs, sizes = (C.c_void_p * 25)(), (C.c_int64 * 10)()
        lib.midas_sites_tables_columns(h, ptrs, sizes)
        col = lambda k, n, dt: np.asarray(_Column(self._owner, ptrs[k] or 0, n, dt))
        rows = (self.n_samples, self.n_sites, self.n_sites, self.n_sites, self.n_sites, self.n_sites, self.n_sites, self.n_genes,
                self.n_columns)
        self._str = {}
        for k, name in enumerate(self.STRING_COLUMNS):
            self._str[name] = (col(2 * k, int(sizes[k]), np.uint8), col(2 * k + 1, rows[k] + 1, np.int64))
        self.mean_coverage = col(18, self.n_samples, np.float64)
        self.fraction_covered = col(19, self.n_samples, np.float64)
        self.gene = col(20, self.n_sites, np.int32)
        self.freq_text = col(21, int(counts[4]), np.uint8)
        self.depth_text = col(22, int(counts[5]), np.uint8)
        self._positions = None

    def _read_positions(self):
        """midas_sites_tables_positions, on the first use of .contig / .ref_pos / .contig_names: a directory without the two
        columns opens as before, and only the command that wants positions hears of it (MidasSnpsError, file and line)."""
        if self._positions is None:
            ptrs, sizes = (C.c_void_p * 4)(), (C.c_int64 * 2)()
            err = C.create_string_buffer(1024)
            st = self._owner._lib.midas_sites_tables_positions(self._owner._h, ptrs, sizes, err)
            if st != 0:
                raise MidasSnpsError(st, err.value.decode(errors='replace') or "midas_sites_tables_positions failed")
            col = lambda k, n, dt: np.asarray(_Column(self._owner, ptrs[k] or 0, n, dt))
            pool, off = col(2, int(sizes[1]), np.uint8), col(3, int(sizes[0]) + 1, np.int64)
            raw = pool.tobytes()
            names = [raw[int(off[k]):int(off[k + 1])].decode('utf-8', errors='surrogateescape') for k in range(int(sizes[0]))]
            self._positions = (col(0, self.n_sites, np.int32), col(1, self.n_sites, np.int64), names)
        return self._positions

    @property
    def contig(self):
        """Per row of snps_info.txt: the index of its ref_id among .contig_names (int32)."""
        return self._read_positions()[0]

    @property
    def ref_pos(self):
        """Per row of snps_info.txt: int(ref_pos) (int64)."""
        return self._read_positions()[1]

    @property
    def contig_names(self):
        """The ref_ids in order of first appearance."""
        return self._read_positions()[2]

    def column(self, name: str):
        """(pool uint8, offsets int64) of a string column."""
        return self._str[name]

    def strings(self, name: str) -> list:
        pool, off = self._str[name]
        text = pool.tobytes().decode('utf-8', errors='surrogateescape')
        if len(text) == pool.shape[0]:
            return [text[int(off[k]):int(off[k + 1])] for k in range(off.shape[0] - 1)]
        raw = pool.tobytes()
        return [raw[int(off[k]):int(off[k + 1])].decode('utf-8', errors='surrogateescape') for k in range(off.shape[0] - 1)]

    def equals(self, name: str, value: str) -> np.ndarray:
        """Per row: the string column equals value (bool), without building Python strings."""
        pool, off = self._str[name]
        v = np.frombuffer(value.encode(), np.uint8)
        n = off.shape[0] - 1
        hit = (off[1:] - off[:-1]) == v.shape[0]
        for k in range(v.shape[0]):
            idx = np.minimum(off[:-1] + k, max(pool.shape[0] - 1, 0))
            hit &= (pool[idx] == v[k]) if pool.shape[0] else np.zeros(n, bool)
        return hit

    def write_markers(self, path: str, rows7):
        """The table of strain_tracking.py id_markers (midas_sites_write_markers): rows7 int32 [n, 7] as Context.sites_id_markers
        returns them."""
        rows = np.ascontiguousarray(rows7, dtype=np.int32).reshape(-1, 7)
        err = C.create_string_buffer(1024)
        st = self._owner._lib.midas_sites_write_markers(path.encode(), self._owner._h, rows.shape[0], rows.ctypes.data_as(C.c_void_p), err)
        if st != 0:
            raise MidasSnpsError(st, err.value.decode(errors='replace') or "midas_sites_write_markers failed")

    def write_pairs(self, path: str, sample_rows, both):
        """The table of strain_tracking.py track_markers (midas_sites_write_pairs): both int64 [S, S] as Context.sites_track_markers
        returns it, sample_rows [S] = the samples' rows of snps_summary.txt."""
        rows = np.ascontiguousarray(sample_rows, dtype=np.int32)
        b = np.ascontiguousarray(both, dtype=np.int64)
        assert b.shape == (rows.shape[0], rows.shape[0])
        err = C.create_string_buffer(1024)
        st = self._owner._lib.midas_sites_write_pairs(path.encode(), self._owner._h, rows.shape[0], rows.ctypes.data_as(C.c_void_p),
                                                      b.ctypes.data_as(C.c_void_p), err)
        if st != 0:
            raise MidasSnpsError(st, err.value.decode(errors='replace') or "midas_sites_write_pairs failed")

    def first_bytes(self, name: str):
        """(first byte of every string, or 0 for an empty one; the lengths)."""
        pool, off = self._str[name]
        ln = off[1:] - off[:-1]
        if pool.shape[0] == 0:
            return np.zeros(ln.shape[0], np.uint8), ln
        first = pool[np.minimum(off[:-1], pool.shape[0] - 1)].copy()
        first[ln == 0] = 0
        return first, ln


GENES_DTYPES = {'presabs': 0, 'copynum': 1}                            # MIDAS_GENES_PRESABS / _COPYNUM
GENES_DISTANCES = {'jaccard': 0, 'euclidean': 1, 'manhattan': 2}       # MIDAS_GENES_JACCARD / _EUCLIDEAN / _MANHATTAN


class GenesMatrix:
    """One genes_<kind>.txt of `merge_midas.py genes` (midas_genes_matrix_*): mapped, not parsed.  .first_field and .sample_ids
    from the header line, .n_rows data rows, .text the rows after the header (uint8 view owned by the handle)."""

    def __init__(self, path: str):
        lib = load_library()
        h = C.c_void_p()
        err = C.create_string_buffer(1024)
        st = lib.midas_genes_matrix_open(path.encode(), C.byref(h), err)
        if st != 0:
            raise MidasSnpsError(st, err.value.decode(errors='replace') or "midas_genes_matrix_open failed")
        self._owner = _GenesOwner(lib, h, 'midas_genes_matrix_close')
        self.path = path
        counts = (C.c_int64 * 4)()
        lib.midas_genes_matrix_counts(h, counts)
        self.n_columns, self.n_rows = int(counts[0]), int(counts[1])
        ptrs, nfirst = (C.c_void_p * 4)(), C.c_int64(0)
        lib.midas_genes_matrix_columns(h, ptrs, C.byref(nfirst))
        col = lambda k, n, dt: np.asarray(_Column(self._owner, ptrs[k] or 0, n, dt))
        pool = col(0, int(counts[3]), np.uint8).tobytes()
        off = col(1, self.n_columns + 1, np.int64)
        self.sample_ids = [pool[int(off[k]):int(off[k + 1])].decode('utf-8', errors='surrogateescape') for k in range(self.n_columns)]
        self.text = col(2, int(counts[2]), np.uint8)
        self.first_field = C.string_at(ptrs[3], nfirst.value).decode('utf-8', errors='surrogateescape') if nfirst.value else ''

    def write_pairs(self, path: str, res: dict):
        """The table of compare_genes.py (midas_genes_compare_write_pairs) from what Context.genes_compare returned."""
        p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None
        arr = lambda k, dt: None if res.get(k) is None else np.ascontiguousarray(res[k], dtype=dt)
        count, both, either, dist = arr('count', np.int64), arr('both', np.float64), arr('either', np.float64), arr('dist', np.float64)
        err = C.create_string_buffer(1024)
        st = self._owner._lib.midas_genes_compare_write_pairs(path.encode(), self._owner._h, int(res['n_samples']), GENES_DTYPES[res['dtype']],
                                                              GENES_DISTANCES[res['distance']], int(res['n_rows']), p(count), p(both),
                                                              p(either), p(dist), err)
        if st != 0:
            raise MidasSnpsError(st, err.value.decode(errors='replace') or "midas_genes_compare_write_pairs failed")

    def write_linkage(self, path: str, res: dict):
        """The pair table of gene_linkage.py (midas_genes_linkage_write_pairs) from what Context.genes_linkage returned."""
        p = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None
        arr = lambda k: np.ascontiguousarray(res[k], dtype=np.int32)
        count, row, a, b, both = arr('count'), arr('row_of_slot'), arr('pair_a'), arr('pair_b'), arr('pair_both')
        err = C.create_string_buffer(1024)
        st = self._owner._lib.midas_genes_linkage_write_pairs(path.encode(), self._owner._h, count.shape[0], p(count), p(row), a.shape[0],
                                                              p(a), p(b), p(both), err)
        if st != 0:
            raise MidasSnpsError(st, err.value.decode(errors='replace') or "midas_genes_linkage_write_pairs failed")

    def write_groups(self, path: str, res: dict, min_group: int = 2) -> int:
        """The group table of gene_linkage.py (midas_genes_linkage_write_groups) -> the groups written."""
        p = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None
        arr = lambda k: np.ascontiguousarray(res[k], dtype=np.int32)
        count, row, label = arr('count'), arr('row_of_slot'), arr('label')
        err, n = C.create_string_buffer(1024), C.c_int64(0)
        st = self._owner._lib.midas_genes_linkage_write_groups(path.encode(), self._owner._h, count.shape[0], p(count), p(row), p(label),
                                                               int(min_group), C.byref(n), err)
        if st != 0:
            raise MidasSnpsError(st, err.value.decode(errors='replace') or "midas_genes_linkage_write_groups failed")
        return int(n.value)

    def write_assoc(self, path: str, res: dict, table: dict):
        """The table of gene_assoc.py (midas_genes_assoc_write) from what Context.genes_assoc returned and the host's columns:
        table = dict(effect, p_value, q_value f64 [K] and, with permutations, p_perm, q_perm)."""
        p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None
        i32a = lambda k: np.ascontiguousarray(res[k], dtype=np.int32)
        f64a = lambda k: None if table.get(k) is None else np.ascontiguousarray(table[k], dtype=np.float64)
        row, count, case = i32a('row_of_slot'), i32a('count'), i32a('count_case')
        P = int(res['n_perms'])
        exceed = np.ascontiguousarray(res['exceed'], dtype=np.uint32) if P else None
        cols = [f64a(k) for k in ('effect', 'p_value', 'q_value', 'p_perm', 'q_perm')]
        err = C.create_string_buffer(1024)
        st = self._owner._lib.midas_genes_assoc_write(path.encode(), self._owner._h, row.shape[0], p(row), p(count), p(case), p(cols[0]),
                                                      p(cols[1]), p(cols[2]), P, p(exceed), p(cols[3]), p(cols[4]), err)
        if st != 0:
            raise MidasSnpsError(st, err.value.decode(errors='replace') or "midas_genes_assoc_write failed")


def pandas_cell(text: bytes):
    """A matrix cell as pandas' C reader converts it, by the library's host build of the device converter
    (midas_genes_compare_parse_cell) -> (value, plain_int), or None when it is no finite decimal literal."""
    lib = load_library()
    out, plain = C.c_double(0), C.c_int32(0)
    if lib.midas_genes_compare_parse_cell(text, len(text), C.byref(out), C.byref(plain)) != 0:
        return None
    return float(out.value), bool(plain.value)


def parse_cell(text: bytes, kind: str):
    """float() ('freq') or int() ('depth') of a matrix cell by the library's exact host parser; None when it is no number."""
    lib = load_library()
    if kind == 'freq':
        out = C.c_double(0)
        return float(out.value) if lib.midas_sites_parse_cell(0, text, len(text), C.byref(out)) == 0 else None
    out = C.c_int64(0)
    return int(out.value) if lib.midas_sites_parse_cell(1, text, len(text), C.byref(out)) == 0 else None


def write_bam(path, ref_names, ref_lengths, refid, reads, level=6, threads=0):
    """The native BAM writer (midas_bam_write): records in the given order, names "r<i>", aux NM + YT:Z:UU -- the bytes of
    midas_amd/bam.py's pure-Python writer, made by all cores."""
    lib = load_library()
    names = (C.c_char_p * len(ref_names))(*[n.encode() for n in ref_names])
    lens = np.ascontiguousarray(ref_lengths, np.int64)
    rid = np.ascontiguousarray(refid, np.int32)
    r = reads._c()
    err = C.create_string_buffer(256)
    st = lib.midas_bam_write(path.encode(), len(ref_names), names, lens.ctypes.data_as(C.c_void_p), C.byref(r),
                             rid.ctypes.data_as(C.c_void_p), int(level), int(threads), err)
    if st != 0:
        raise MidasSnpsError(st, err.value.decode())


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


class BamSlice:
    """Rank-local view of a BAM (midas_bam_open_slice): this rank's share of the file walked, facts to exchange with the
    other ranks, then only the record ranges this rank owns decoded (midas_bam_load_ranges)."""

    def __init__(self, path: str, slice_index: int, n_slices: int, ctx=None):
        """ctx (a Context): the slice's blocks are inflated and walked on its device (midas_bam_open_slice_device)."""
        self._lib = load_library()
        h = C.c_void_p()
        err = C.create_string_buffer(256)
        if ctx is not None and getattr(ctx, 'inflates', False):
            st = self._lib.midas_bam_open_slice_device(path.encode(), int(slice_index), int(n_slices), ctx._h, C.byref(h), err)
        else:
            st = self._lib.midas_bam_open_slice(path.encode(), int(slice_index), int(n_slices), C.byref(h), err)
        if st != 0:
            raise MidasSnpsError(st, err.value.decode())
        self._h = h
        self.ref_names, self.ref_lens = _bam_refs(self._lib, h)
        n = len(self.ref_names)
        out7 = np.zeros(7, np.int64)
        self.ref_reads, self.ref_bases, self.ref_first = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
        p = lambda x: x.ctypes.data_as(C.c_void_p)
        self._lib.midas_bam_slice_facts(h, p(out7), p(self.ref_reads), p(self.ref_bases), p(self.ref_first))
        (self.first, self.end, self.sorted, self.first_ref, self.last_ref, self.rec_begin, self.total) = (int(x) for x in out7)

    def marks(self):
        """(pos_sorted, first_pos, last_pos, ref_span int64 [n_ref], marks int64 [n, 3] = refID, bin, offset): what a
        contig needs to be cut into pieces (midas_bam_slice_marks)."""
        p = lambda x: x.ctypes.data_as(C.c_void_p)
        out4 = np.zeros(4, np.int64)
        span = np.zeros(len(self.ref_names), np.int64)
        self._lib.midas_bam_slice_marks(self._h, p(out4), p(span), None, 0)
        marks = np.zeros((int(out4[3]), 3), np.int64)
        if marks.size:
            self._lib.midas_bam_slice_marks(self._h, p(out4), None, p(marks), marks.shape[0])
        return int(out4[0]), int(out4[1]), int(out4[2]), span, marks

    def load_ranges(self, ranges, ctx=None, resident: bool = False):
        """[(begin, end)] uncompressed record ranges -> (refid int32, ReadsSoA) of the records in them, in file order.
        ctx (a Context): the ranges are decoded on its device and SEQ / QUAL / CIGAR stay there (midas_bam_load_ranges_device):
        the ReadsSoA carries their device addresses (`device`), as read_bam(..., payload_on_device=True)'s does."""
        rb = np.array([r[0] for r in ranges], np.int64)
        re_ = np.array([r[1] for r in ranges], np.int64)
        n, sb, qb, nc = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        err = C.create_string_buffer(256)
        p = lambda x: x.ctypes.data_as(C.c_void_p)
        if resident and ctx is not None and getattr(ctx, 'inflates', False) and len(ranges):
            # (everything stays on the device, in the direct layout: read_bam(..., resident=True)'s form for a rank's ranges)
            total = C.c_int64()
            st = self._lib.midas_bam_load_ranges_resident(self._h, ctx._h, len(ranges), p(rb), p(re_), C.byref(n), C.byref(total), err)
            if st == 0 and self._lib.midas_bam_is_resident(self._h):
                keeper = _BamOwner(self._lib, None)
                keeper._slice = self
                ptrs = (C.c_void_p * 12)()
                self._lib.midas_bam_columns(self._h, ptrs)
                refid = np.asarray(_Column(keeper, ptrs[0] or 0, int(n.value), np.int32))
                return refid, ResidentReads(self._lib, self._h, keeper, int(n.value), int(total.value))
            if st != ERR_UNSUPPORTED:
                if st != 0:
                    raise MidasSnpsError(st, err.value.decode())
        if ctx is not None and getattr(ctx, 'inflates', False):
            st = self._lib.midas_bam_load_ranges_device(self._h, ctx._h, len(ranges), p(rb), p(re_), C.byref(n), C.byref(sb),
                                                        C.byref(qb), C.byref(nc), err)
        else:
            st = self._lib.midas_bam_load_ranges(self._h, len(ranges), p(rb), p(re_), C.byref(n), C.byref(sb), C.byref(qb),
                                                 C.byref(nc), err)
        if st != 0:
            raise MidasSnpsError(st, err.value.decode())
        keeper = _BamOwner(self._lib, None)
        keeper._slice = self                # the arrays keep this object (and with it the native handle) alive
        return _bam_columns(self._lib, self._h, int(n.value), int(sb.value), int(qb.value), int(nc.value), keeper,
                            on_device=bool(self._lib.midas_bam_payload_on_device(self._h)))

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
        err = C.create_string_buffer(256)
        out3 = np.zeros(3, np.int64)
        st = self._lib.midas_bam_open_share(path.encode(), int(slice_index), int(n_slices), int(max_walk), C.byref(h),
                                            out3.ctypes.data_as(C.c_void_p), err)
        if st != 0:
            raise MidasSnpsError(st, err.value.decode())
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
        err = C.create_string_buffer(256)
        out4 = np.zeros(4, np.int64)
        st = self._lib.midas_bam_open_share_local(path.encode(), int(slice_index), int(n_slices), C.byref(h),
                                                  out4.ctypes.data_as(C.c_void_p), err)
        if st != 0:
            raise MidasSnpsError(st, err.value.decode())
        self._h, self._slice = h, int(slice_index)
        self.ref_names, self.ref_lens = _bam_refs(self._lib, h)
        self.walk = tuple(int(x) for x in out4)
        self.first = self.total = self.rec_begin = -1
        return self

    def locate(self, upos_base: int, total: int, max_walk: int = 256 << 20):
        out3 = np.zeros(3, np.int64)
        err = C.create_string_buffer(256)
        st = self._lib.midas_bam_share_locate(self._h, self._slice, int(upos_base), int(total), int(max_walk),
                                              out3.ctypes.data_as(C.c_void_p), err)
        if st != 0:
            raise MidasSnpsError(st, err.value.decode())
        self.first, self.total, self.rec_begin = (int(x) for x in out3)
        return self


class PinnedPool:
    """Page-locked result buffers of a Context (midas_snps_host_alloc): grown on demand and REUSED across calls -- pinning
    a quarter of a gigabyte costs more than the copy it speeds up.  An array handed out under a key is overwritten by the
    next request for that key."""

    def __init__(self, lib):
        self._lib = lib
        self._bufs = {}

    def array(self, key, shape, dtype):
        dtype = np.dtype(dtype)
        nbytes = max(1, int(np.prod(shape)) * dtype.itemsize)
        ptr, cap = self._bufs.get(key, (None, 0))
        if cap < nbytes:
            if ptr:
                self._lib.midas_snps_host_free(C.c_void_p(ptr))
            ptr = self._lib.midas_snps_host_alloc(nbytes)
            if not ptr:
                self._bufs.pop(key, None)
                return np.empty(shape, dtype)          # no pinned memory: an ordinary array (staged copy)
            self._bufs[key] = (ptr, nbytes)
        return np.frombuffer((C.c_uint8 * nbytes).from_address(ptr), dtype=dtype, count=int(np.prod(shape))).reshape(shape)

    def close(self):
        for ptr, _ in self._bufs.values():
            self._lib.midas_snps_host_free(C.c_void_p(ptr))
        self._bufs = {}


class Context:
    """One GPU.  Replaces a `mp.Pool` worker and its module globals (midas/run/snps.py:142,167-176)."""

    def __init__(self, device: int = 0):
        self._lib = load_library()
        self._pool = None
        h = C.c_void_p()
        st = self._lib.midas_snps_create(int(device), C.byref(h))
        if st != 0:
            raise MidasSnpsError(st, "midas_snps_create(device=%d): %s"
                                 % (device, self._lib.midas_snps_status_string(st).decode()))
        self._h = h
        self.device = int(device)

    def close(self):
        if getattr(self, '_pool', None):
            self._pool.close()
            self._pool = None
        if getattr(self, '_h', None):
            self._lib.midas_snps_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def pinned(self, key, shape, dtype):
        """A page-locked array owned by the context (see PinnedPool): valid until the same key is asked for again."""
        if self._pool is None:
            self._pool = PinnedPool(self._lib)
        return self._pool.array(key, shape, dtype)

    def _check(self, st: int):
        if st != 0:
            msg = self._lib.midas_snps_last_error(self._h).decode() or \
                self._lib.midas_snps_status_string(st).decode()
            raise MidasSnpsError(st, msg, int(self._lib.midas_snps_last_error_read(self._h)))

    def _check_bad(self, st: int, stats):
        """_check() for a call that reports the place of a bad row: the error carries .bad = stats[4..6], None where [4] is 0."""
        try:
            self._check(st)
        except MidasSnpsError as e:
            e.bad = (int(stats[4]), int(stats[5]), int(stats[6])) if stats[4] else None
            raise

    def set_stream(self, hip_stream: Optional[int]):
        self._check(self._lib.midas_snps_set_stream(self._h, C.c_void_p(hip_stream or 0)))

    def set_default_path(self, path: int):
        """The path of every batch created on this context from now on (PATH_AUTO: each batch's own choice)."""
        self._check(self._lib.midas_snps_set_default_path(self._h, int(path)))

    def set_pad_rule(self, rule: int):
        """PAD_SPEC (default): the CIGAR op P consumes nothing; PAD_PYSAM: it advances the query position, as
        get_aligned_pairs of the pysam releases of MIDAS's time does.  For batches created afterwards."""
        self._check(self._lib.midas_snps_set_pad_rule(self._h, int(rule)))

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
        p = lambda x: x.ctypes.data_as(C.c_void_p)
        crc = None if crc is None else np.ascontiguousarray(crc, np.uint32)
        st = self._lib.midas_snps_inflate_blocks(self._h, p(comp), comp.size, cpos.size, p(cpos), p(clen), p(upos), p(ulen),
                                                 None if crc is None else p(crc), p(out), int(out_bytes), C.byref(bad))
        if st != 0:
            msg = self._lib.midas_snps_last_error(self._h).decode() or self._lib.midas_snps_status_string(st).decode()
            raise MidasSnpsError(st, msg, int(bad.value))
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
            self._check(self._lib.midas_snps_copy_from_device(self._h, buf.ctypes.data_as(C.c_void_p), C.c_void_p(int(src)), s))
        d = reads.as_dict()
        d.update(seq4=out[0][:sizes[0]], qual=out[1][:sizes[1]], cigar=out[2][:sizes[2]].view(np.uint32))
        return ReadsSoA(**d)

    def set_row_coder(self, coder: int):
        """ROWS_DEVICE (default): Batch.write_part formats and deflates the rows in a kernel; ROWS_HOST: the host's
        formatter threads do (the file then equals write_table's byte for byte).  Same text either way."""
        self._check(self._lib.midas_snps_set_row_coder(self._h, int(coder)))

    def row_coder_counts(self):
        """Who coded the parts Batch.write_part wrote on this context (midas_snps_row_coder_counts): members coded by the kernel,
        parts left to the host's formatter for a contig id beyond 192 bytes, parts left to it for a member the kernel declined."""
        out = np.zeros(3, np.int64)
        self._check(self._lib.midas_snps_row_coder_counts(self._h, out.ctypes.data_as(C.c_void_p)))
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
        p = lambda x: x.ctypes.data_as(C.c_void_p)
        self._check(self._lib.midas_snps_rows_code(self._h, allele.size, p(counts), p(allele), n, p(site0), p(pos0), p(n_rows), p(id_off),
                                                   p(id_len), p(ids), ids.size - 1, int(arena_bytes), int(grid_blocks), p(st_), p(nb),
                                                   p(crc), p(tl), p(off), p(streams), streams.size, C.byref(got)))
        out, at = [], 0
        for k in range(n):
            stream = None
            if st_[k] == 0:
                stream = streams[at:at + int(nb[k])].tobytes()
                at += int(nb[k])
            out.append(dict(status=int(st_[k]), n_bytes=int(nb[k]), crc=int(crc[k]), text_len=int(tl[k]), arena_off=int(off[k]), stream=stream))
        assert at == got.value
        return out

    def scan_u32(self, v, in_place: bool = False, n=None):
        """The library's exclusive scan of 32-bit counters on v, between guard words (midas_snps_scan_u32; test aid).
        in_place: one device buffer is input and output.  n: the count handed over, len(v) unless given.
        -> (out uint32 [n], guards_ok, in_kept)."""
        v = np.ascontiguousarray(v, np.uint32).reshape(-1)
        out = np.zeros(v.size, np.uint32)
        ok, kept = C.c_int32(-1), C.c_int32(-1)
        p = lambda x: x.ctypes.data_as(C.c_void_p)
        self._check(self._lib.midas_snps_scan_u32(self._h, v.size if n is None else int(n), p(v), int(bool(in_place)), p(out),
                                                  C.byref(ok), C.byref(kept)))
        return out, ok.value == 1, kept.value == 1

    def sort_pairs(self, key, val, bits: int, n=None):
        """The library's stable radix sort of (key, val) pairs by the keys' low `bits` bits, between guard words
        (midas_snps_sort_pairs; test aid).  key uint32 [n] below 2^bits; val uint32 [n] or float64 [n] (moved as bit patterns).
        n: the count handed over, len(key) unless given.
        -> (keys, values, which, guards_ok); which: 0 the result lay in the buffer pair the input went up to, 1 in the other."""
        key = np.ascontiguousarray(key, np.uint32).reshape(-1)
        val = np.ascontiguousarray(val).reshape(-1)
        if val.dtype not in (np.uint32, np.float64) or val.size != key.size:
            raise ValueError("sort_pairs: val must be uint32 or float64 and as long as key")
        out_key, out_val = np.zeros(key.size, np.uint32), np.zeros(val.size, val.dtype)
        which, ok = C.c_int32(-1), C.c_int32(-1)
        p = lambda x: x.ctypes.data_as(C.c_void_p)
        self._check(self._lib.midas_snps_sort_pairs(self._h, key.size if n is None else int(n), int(bits), int(val.dtype == np.float64),
                                                    p(key), p(val), p(out_key), p(out_val), C.byref(which), C.byref(ok)))
        return out_key, out_val, which.value, ok.value == 1

    def mt19937_stream(self, key, pos: int, n_words: int, per_launch: int = 0, bound: int = 0xFFFFFFFF):
        """The device's MT19937 generator from numpy's legacy state (key uint32 [624], pos), n_words words, per_launch a launch
        (midas_snps_mt19937_stream; test aid).  -> (raw uint32 [n], accepted uint8 [n], masked uint32 [n], key uint32 [624], pos)."""
        key = np.ascontiguousarray(key, np.uint32).reshape(-1)
        assert key.size == 624
        n = int(n_words)
        raw, flag, masked = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.uint32)
        key_out, pos_out = np.zeros(624, np.uint32), C.c_int32(-1)
        p = lambda x: x.ctypes.data_as(C.c_void_p)
        self._check(self._lib.midas_snps_mt19937_stream(self._h, p(key), int(pos), n, int(per_launch), int(bound), p(raw), p(flag), p(masked),
                                                        p(key_out), C.byref(pos_out)))
        return raw[:n], flag[:n], masked[:n], key_out, pos_out.value

    def copy_rate(self, nbytes: int = 1 << 30, reps: int = 10) -> float:
        """GB/s (read + written) of a device-to-device copy with the library's 16-bytes-per-lane copy kernel."""
        out = C.c_double(0.0)
        self._check(self._lib.midas_snps_copy_rate(self._h, int(nbytes), int(reps), C.byref(out)))
        return out.value

    def stream_rates(self, nbytes: int = 1 << 32, reps: int = 5):
        """GB/s of a saturating read stream, write stream and copy (read + written) over nbytes per buffer."""
        out = (C.c_double * 3)()
        self._check(self._lib.midas_snps_stream_rates(self._h, int(nbytes), int(reps), out))
        return {"read_GBps": out[0], "write_GBps": out[1], "copy_GBps": out[2]}

    def calibration_pass(self, nbytes: int = 1 << 30):
        """The known-byte-count kernels that calibrate FETCH_SIZE / WRITE_SIZE (run it under rocprofv3 --pmc)."""
        self._check(self._lib.midas_snps_calibration_pass(self._h, int(nbytes)))

    def device_info(self):
        name = C.create_string_buffer(256)
        ncu = C.c_int32(0)
        mem = C.c_int64(0)
        self._check(self._lib.midas_snps_device_info(self._h, name, C.byref(ncu), C.byref(mem)))
        return {'name': name.value.decode(), 'compute_units': ncu.value, 'hbm_bytes': mem.value}

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
        st = self._lib.midas_snps_pileup(self._h, C.byref(thr), C.byref(c), C.byref(r),
                                         counts.ctypes.data_as(C.c_void_p),
                                         allele.ctypes.data_as(C.c_void_p) if want_allele else None,
                                         stats.ctypes.data_as(C.c_void_p))
        self._check(st)
        return counts, allele, stats

    def genes_count(self, thr: Thresholds, reads: "ReadsSoA", ref_id, gene_length):
        """midas_genes_count(): per gene (aligned_reads i64, mapped_reads i64, depth f64, kernel_ms)."""
        rid = np.ascontiguousarray(ref_id, dtype=np.int32)
        gl = np.ascontiguousarray(gene_length, dtype=np.int64)
        n = gl.shape[0]
        aligned, mapped, depth = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.float64)
        ms = C.c_float(0)
        r = reads._c()
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        st = self._lib.midas_genes_count(self._h, C.byref(thr), C.byref(r), p(rid), n, p(gl), p(aligned), p(mapped), p(depth),
                                         C.byref(ms))
        self._check(st)
        return aligned, mapped, depth, float(ms.value)

    def genes_count_device(self, thr: Thresholds, reads: "ReadsSoA", ref_id, gene_length):
        """midas_genes_count_device(): genes_count over a ReadsSoA whose QUAL / CIGAR lie on this context's device (read_sam(...,
        order='file'), read_bam(..., payload_on_device=True), BamSlice.load_ranges(ctx=...)); the per-read facts are made there."""
        if isinstance(reads, ResidentReads):
            reads = reads.to_columns(self)
        if reads.device is None:
            raise MidasSnpsError(ERR_INVALID_ARG, "genes_count_device takes reads whose payload is on the device (genes_count takes host columns)")
        rid = np.ascontiguousarray(ref_id, dtype=np.int32)
        gl = np.ascontiguousarray(gene_length, dtype=np.int64)
        n = gl.shape[0]
        aligned, mapped, depth = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.float64)
        ms = C.c_float(0)
        r = reads._c()
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        st = self._lib.midas_genes_count_device(self._h, C.byref(thr), C.byref(r), p(rid), n, p(gl), p(aligned), p(mapped), p(depth),
                                                C.byref(ms))
        self._check(st)
        return aligned, mapped, depth, float(ms.value)

    def genes_count_timing(self) -> dict:
        """Device milliseconds of the last genes_count_device on this context (midas_genes_count_timing), by phase."""
        ms = (C.c_float * 2)()
        self._check(self._lib.midas_genes_count_timing(self._h, ms))
        return {'facts kernel': float(ms[0]), 'filter + sort + sums': float(ms[1])}

    def genes_count_bam(self, thr: Thresholds, handle: "BamDeviceHandle", gene_length):
        """midas_genes_count_bam(): genes_count over the BAM behind `handle` (open_bam_device) in one pass on this context's device;
        gene_length[i]: the length of reference i of the header.  -> (aligned_reads i64, mapped_reads i64, depth f64, ms: the
        call's device milliseconds from the inflate to the download)."""
        gl = np.ascontiguousarray(gene_length, dtype=np.int64)
        n = gl.shape[0]
        aligned, mapped, depth = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.float64)
        stats, ms = np.zeros(8, np.int64), np.zeros(8, np.float32)
        err = C.create_string_buffer(256)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        st = self._lib.midas_genes_count_bam(self._h, handle._h, C.byref(thr), n, p(gl), p(aligned), p(mapped), p(depth), p(stats), p(ms), err)
        self._genes_bam = (dict(zip(GENES_BAM_PHASES, (float(x) for x in ms))), dict(zip(GENES_BAM_STATS, (int(x) for x in stats))))
        self._check(st)
        return aligned, mapped, depth, float(ms[1:6].sum())

    def genes_count_bam_timing(self):
        """(laps, stats) of the last genes_count_bam on this context: milliseconds by phase (GENES_BAM_PHASES: the upload by the host's
        clock, the others device events) and the decode's counts (GENES_BAM_STATS)."""
        if getattr(self, '_genes_bam', None) is None:
            raise MidasSnpsError(ERR_INVALID_ARG, "genes_count_bam_timing: no genes_count_bam has run on this context")
        return self._genes_bam

    def genes_terms(self, thr: Thresholds, reads: "ReadsSoA", ref_id, gene_length):
        """midas_genes_terms(): per read of a slice its term (f64; +0.0 for a read keep_read drops)."""
        rid = np.ascontiguousarray(ref_id, dtype=np.int32)
        gl = np.ascontiguousarray(gene_length, dtype=np.int64)
        term = np.zeros(int(reads.n_reads), np.float64)
        ms = C.c_float(0)
        r = reads._c()
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        st = self._lib.midas_genes_terms(self._h, C.byref(thr), C.byref(r), p(rid), gl.shape[0], p(gl), p(term), C.byref(ms))
        self._check(st)
        return term

    def genes_sum(self, gene, term, n_genes):
        """midas_genes_sum(): (gene, term) pairs in BAM order -> per gene (aligned_reads i64, mapped_reads i64, depth f64)."""
        g = np.ascontiguousarray(gene, dtype=np.int32)
        t = np.ascontiguousarray(term, dtype=np.float64)
        n = int(n_genes)
        aligned, mapped, depth = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.float64)
        ms = C.c_float(0)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        st = self._lib.midas_genes_sum(self._h, g.shape[0], p(g), p(t), n, p(aligned), p(mapped), p(depth), C.byref(ms))
        self._check(st)
        return aligned, mapped, depth

    def parse_rows(self, text: bytes, skip_header: bool = True, cap_rows: int = None):
        """The device's row parser on the text of one table (midas_snps_parse_rows_device) -> (counts[n,4] u32 of the first cap_rows
        rows, rows found, first malformed row among them or -1)."""
        buf = np.frombuffer(text, np.uint8)
        cap = int(cap_rows) if cap_rows is not None else text.count(b"\n") + 1
        out = np.zeros((cap, 4), np.uint32)
        rows, bad = C.c_int64(0), C.c_int64(-1)
        self._check(self._lib.midas_snps_parse_rows_device(self._h, buf.ctypes.data_as(C.c_void_p) if buf.size else None, buf.size, 1 if skip_header else 0,
                                                           out.ctypes.data_as(C.c_void_p), cap, C.byref(rows), C.byref(bad)))
        return out[:min(cap, int(rows.value))], int(rows.value), int(bad.value)

    def read_snps_counts_device(self, paths, row_begin: int = 0, max_rows: int = -1, first_slot: int = 0, extra_slots: int = 0):
        """The count columns of several samples' <species>.snps.gz inflated and parsed on the device
        (midas_snps_tableset_read_counts_device) -> MergeTables: table k of `paths` in sample slot first_slot + k, rows
        [row_begin, max_rows) of the SHORTEST table (max_rows < 0: its end), as read_snps_counts.  first_slot / extra_slots: slots in
        front of / behind the tables' for samples the caller fills (MergeTables.set_host).  Raises MidasSnpsError: ERR_UNSUPPORTED
        when a file does not announce its rows, ERR_BAD_LAYOUT (naming the file) when one is corrupt; nothing stays allocated."""
        lib = self._lib
        n = len(paths)
        arr = (C.c_char_p * n)(*[p.encode() for p in paths])
        rows = np.empty(n, np.int64)
        h = C.c_void_p()
        err = C.create_string_buffer(256)
        st = lib.midas_snps_tableset_open(n, arr, C.byref(h), rows.ctypes.data_as(C.c_void_p), err)
        if st != 0:
            raise MidasSnpsError(st, err.value.decode())
        try:
            if (rows < 0).any():
                raise MidasSnpsError(ERR_UNSUPPORTED, "%s: the file does not announce its rows" % paths[int(np.nonzero(rows < 0)[0][0])])
            hi = int(rows.min()) if max_rows < 0 else min(int(rows.min()), int(max_rows))
            m = max(0, hi - int(row_begin))
            tables = MergeTables(self, int(first_slot) + n + int(extra_slots), m)
            stats, ms = np.zeros(8, np.int64), np.zeros(4, np.float32)
            st = lib.midas_snps_tableset_read_counts_device(self._h, h, int(row_begin), m, int(first_slot), tables._h, stats.ctypes.data_as(C.c_void_p),
                                                            ms.ctypes.data_as(C.c_void_p), err)
            if st != 0:
                tables.close()
                raise MidasSnpsError(st, err.value.decode())
            tables.stats = dict(zip(TABLES_READ_STATS, (int(x) for x in stats)))
            tables.ms = dict(zip(TABLES_READ_PHASES, (float(x) for x in ms)))
            return tables
        finally:
            lib.midas_snps_tableset_close(h)

    def _merge_resident(self, prm, tables: "MergeTables", mean_depth, with_matrices: bool):
        n, S = tables.n_sites, tables.n_samples
        md = np.ascontiguousarray(mean_depth, dtype=np.float64)
        assert md.shape == (S,)
        calls = np.empty((n, 4), np.uint8)
        out = dict(major=calls[:, 0], minor=calls[:, 1], snp_type=calls[:, 2], flag=calls[:, 3],
                   count_samples=np.empty(n, np.uint32), pooled=np.empty((n, 4), np.uint64))
        if with_matrices:
            out.update(depth=np.empty((S, n), np.uint32), minor_count=np.empty((S, n), np.uint32))
        return n, md, calls, out

    def merge_sites(self, prm: "MergeParams", sample_counts, mean_depth):
        """midas_merge_sites(): sample_counts = list of [n_sites,4] uint32 arrays (one per sample), or a MergeTables (the counts
        where the device readers left them: midas_merge_sites_resident).
        -> dict(major, minor, snp_type, flag, count_samples, pooled[n,4] u64, depth[S,n] u32, minor_count[S,n] u32, kernel_ms)"""
        if isinstance(sample_counts, MergeTables):
            n, md, calls, out = self._merge_resident(prm, sample_counts, mean_depth, True)
            ms = C.c_float(0)
            p = lambda a: a.ctypes.data_as(C.c_void_p)
            st = self._lib.midas_merge_sites_resident(self._h, C.byref(prm), sample_counts._h, n, p(md), p(calls), p(out['count_samples']), p(out['pooled']),
                                                      p(out['depth']), p(out['minor_count']), C.byref(ms))
            self._check(st)
            out['kernel_ms'] = float(ms.value)
            return out
        S = len(sample_counts)
        arrs = [np.ascontiguousarray(a, dtype=np.uint32) for a in sample_counts]
        n = arrs[0].shape[0]
        assert all(a.shape == (n, 4) for a in arrs)
        ptrs = (C.c_void_p * S)(*[a.ctypes.data for a in arrs])
        md = np.ascontiguousarray(mean_depth, dtype=np.float64)
        calls = np.empty((n, 4), np.uint8)
        out = dict(major=calls[:, 0], minor=calls[:, 1], snp_type=calls[:, 2], flag=calls[:, 3],
                   count_samples=np.empty(n, np.uint32), pooled=np.empty((n, 4), np.uint64),
                   depth=np.empty((S, n), np.uint32), minor_count=np.empty((S, n), np.uint32))
        ms = C.c_float(0)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        st = self._lib.midas_merge_sites(self._h, C.byref(prm), S, n, ptrs, p(md), p(calls),
                                         p(out['count_samples']), p(out['pooled']),
                                         p(out['depth']), p(out['minor_count']), C.byref(ms))
        self._check(st)
        out['kernel_ms'] = float(ms.value)
        return out

    def merge_sites_tables(self, prm: "MergeParams", sample_counts, mean_depth, freq_path: str, depth_path: str, header_line: str,
                           site_id_base: int = 0):
        """midas_merge_sites_tables(): merge_sites with snps_freq.txt / snps_depth.txt written from the device -- depth and
        minor_count stay there.  -> dict(major, minor, snp_type, flag, count_samples, pooled[n,4] u64, n_keep, kernel_ms,
        format_ms).  sample_counts: the list of arrays, or a MergeTables (midas_merge_sites_tables_resident)."""
        if isinstance(sample_counts, MergeTables):
            n, md, calls, out = self._merge_resident(prm, sample_counts, mean_depth, False)
            ms, fms, kept = C.c_float(0), C.c_float(0), C.c_int64(0)
            p = lambda a: a.ctypes.data_as(C.c_void_p)
            st = self._lib.midas_merge_sites_tables_resident(self._h, C.byref(prm), sample_counts._h, n, p(md), freq_path.encode(), depth_path.encode(),
                                                             header_line.encode(), int(site_id_base), p(calls), p(out['count_samples']),
                                                             p(out['pooled']), C.byref(kept), C.byref(ms), C.byref(fms))
            self._check(st)
            out['n_keep'], out['kernel_ms'], out['format_ms'] = int(kept.value), float(ms.value), float(fms.value)
            return out
        S = len(sample_counts)
        arrs = [np.ascontiguousarray(a, dtype=np.uint32) for a in sample_counts]
        n = arrs[0].shape[0]
        assert all(a.shape == (n, 4) for a in arrs)
        ptrs = (C.c_void_p * S)(*[a.ctypes.data for a in arrs])
        md = np.ascontiguousarray(mean_depth, dtype=np.float64)
        calls = np.empty((n, 4), np.uint8)
        out = dict(major=calls[:, 0], minor=calls[:, 1], snp_type=calls[:, 2], flag=calls[:, 3],
                   count_samples=np.empty(n, np.uint32), pooled=np.empty((n, 4), np.uint64))
        ms, fms, kept = C.c_float(0), C.c_float(0), C.c_int64(0)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        st = self._lib.midas_merge_sites_tables(self._h, C.byref(prm), S, n, ptrs, p(md), freq_path.encode(), depth_path.encode(),
                                                header_line.encode(), int(site_id_base), p(calls), p(out['count_samples']),
                                                p(out['pooled']), C.byref(kept), C.byref(ms), C.byref(fms))
        self._check(st)
        out['n_keep'], out['kernel_ms'], out['format_ms'] = int(kept.value), float(ms.value), float(fms.value)
        return out

    def genes_merge(self, cluster, copy, depth, reads, n_clusters: int, min_copy: float, group_samples: int = 0):
        """midas_genes_merge(): per sample s the cluster index [n_s] uint32 and copy / depth f64 / reads i64 columns of its
        table rows (lists of arrays; samples may share one cluster array).  -> dict(rows [R] uint32 = the clusters sample 0
        mentions, in index order; copy, depth [R, S] f64; reads [R, S] i64; state [R, S] uint8 (0 absent, 1 present below
        min_copy, 2 present at or above); kernel_ms)."""
        S = len(cluster)
        cl = [np.ascontiguousarray(a, dtype=np.uint32) for a in cluster]
        cp = [np.ascontiguousarray(a, dtype=np.float64) for a in copy]
        dp = [np.ascontiguousarray(a, dtype=np.float64) for a in depth]
        rd = [np.ascontiguousarray(a, dtype=np.int64) for a in reads]
        n = np.array([a.shape[0] for a in cl], np.int64)
        assert all(cp[k].shape[0] == n[k] and dp[k].shape[0] == n[k] and rd[k].shape[0] == n[k] for k in range(S))
        ptrs = lambda arrs: (C.c_void_p * S)(*[a.ctypes.data if a.size else None for a in arrs])
        cap = int(min(int(n_clusters), int(n[0]))) if S else 0
        out = dict(rows=np.empty(cap, np.uint32), copy=np.empty((cap, S), np.float64), depth=np.empty((cap, S), np.float64),
                   reads=np.empty((cap, S), np.int64), state=np.empty((cap, S), np.uint8))
        R, ms = C.c_int64(0), C.c_float(0)
        p = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None
        keep = (cl, cp, dp, rd)     # (alive during the call)
        st = self._lib.midas_genes_merge(self._h, S, p(n), ptrs(cl), ptrs(cp), ptrs(dp), ptrs(rd), int(n_clusters), float(min_copy),
                                         int(group_samples), cap, C.byref(R), p(out['rows']), p(out['copy']), p(out['depth']),
                                         p(out['reads']), p(out['state']), C.byref(ms))
        del keep
        self._check(st)
        r = int(R.value)
        res = {k: v[:r] for k, v in out.items()}
        res['kernel_ms'] = float(ms.value)
        return res

    def sites_scan(self, freq_text, depth_text, site_mask, sample_col, mean_depth, site_depth: int, site_ratio: float,
                   allele_support: float, site_prev: float, site_maf: float, snp_maf: float = 0.01, max_sites: int = -1,
                   flags: int = 0, site_gene=None, n_genes: int = 0, minor=None, major=None, group_rows: int = 0,
                   chunk_bytes: int = 0, dump: bool = False, dump_keep: bool = False, rand_reads: int = 0, replace_reads: bool = False,
                   np_state=None, draw_chunk: int = 0, _classes=None):
        """midas_sites_scan(): the per-site loop of snp_diversity.py / call_consensus.py over the text rows of snps_freq.txt
        and snps_depth.txt (uint8 arrays, header line excluded).  site_mask [N] uint8; sample_col / mean_depth [S].  -> dict
        (n_sites, n_kept, side_freq, side_depth, groups, no_gene, ms [8]; with SITES_SUMS pi f64, snps / sites / depth i64
        [chains, genes]; with SITES_SEQ seq uint8 [S, n_kept]; with dump: freq f64 / depthv i64 [S, n_sites], keep uint8 and
        pooled f64 [n_sites]; with dump_keep: keep alone).  A malformed row raises MidasSnpsError with .bad = (matrix 1|2, data row, sample or -1);
        a site the reference raises on, with .bad = (3, data row, sample): a frequency that is not finite under SITES_ROUND, or
        (6, data row, -1): kept samples whose depths sum to 0 under SITES_WEIGHT.
        rand_reads N > 0: midas_sites_scan_resampled(), snp_diversity.py's --rand_reads N [--replace_reads] from numpy's legacy
        generator state np_state (np.random.get_state(); read, not advanced: None takes the global one).  The result also holds
        np_state = the state the reference's loop leaves (for np.random.set_state), n_resampled sites, n_drew cells, raw_made /
        accepted_used / raw_consumed words and draw_ms [5] (eligibility, generation, compaction, resampling, pooled frequencies);
        draw_chunk: the raw words a launch of the generator makes at most (0: chosen; no output depends on it).
        _classes: sites_scan_classes' (site_class or None, n_classes)."""
        ft = np.ascontiguousarray(freq_text, dtype=np.uint8)
        dt = np.ascontiguousarray(depth_text, dtype=np.uint8)
        mask = np.ascontiguousarray(site_mask, dtype=np.uint8)
        N = int(mask.shape[0])
        cols = np.ascontiguousarray(sample_col, dtype=np.int32)
        mean = np.ascontiguousarray(mean_depth, dtype=np.float64)
        S = int(cols.shape[0])
        assert mean.shape[0] == S and S >= 1
        pooled, per_gene = bool(flags & SITES_POOLED), bool(flags & SITES_PER_GENE)
        gene = np.ascontiguousarray(site_gene, dtype=np.int32) if per_gene else None
        assert gene is None or gene.shape[0] == N
        G = int(n_genes) if per_gene else 1
        chains = 1 if pooled else S
        cap = N if max_sites < 0 else min(N, int(max_sites))
        mi = np.ascontiguousarray(minor, dtype=np.uint8) if flags & SITES_SEQ else None
        ma = np.ascontiguousarray(major, dtype=np.uint8) if flags & SITES_SEQ else None
        assert mi is None or (mi.shape[0] == N and ma.shape[0] == N)
        fp = np.array([site_ratio, allele_support, site_prev, site_maf, snp_maf], np.float64)
        ip = np.array([site_depth, max_sites, flags, G if per_gene else 0, group_rows, chunk_bytes, cap, draw_chunk if rand_reads else 0], np.int64)
        out = {}
        if flags & SITES_SUMS:
            shape = (chains, G) if _classes is None else (max(int(_classes[1]), 0), chains, G)
            out.update(pi=np.zeros(shape, np.float64), snps=np.zeros(shape, np.int64), sites=np.zeros(shape, np.int64),
                       depth=np.zeros(shape, np.int64))
        seq = np.empty((S, max(cap, 1)), np.uint8) if flags & SITES_SEQ else None       # (max_sites 0: still a buffer to point at)
        if dump:
            out.update(freq=np.zeros((S, N), np.float64), depthv=np.zeros((S, N), np.int64), keep=np.zeros(N, np.uint8),
                       pooled=np.zeros(N, np.float64))
        elif dump_keep:
            out.update(keep=np.zeros(N, np.uint8))
        stats, ms = np.zeros(16, np.int64), np.zeros(8, np.float32)
        p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None
        common = (self._h, p(ft), ft.shape[0], p(dt), dt.shape[0], N, p(mask), p(gene), p(mi), p(ma), S, p(cols), p(mean), p(fp), p(ip),
                  p(out.get('pi')), p(out.get('snps')), p(out.get('sites')), p(out.get('depth')), p(seq), p(out.get('freq')),
                  p(out.get('depthv')), p(out.get('keep')), p(out.get('pooled')), p(stats), p(ms))
        if rand_reads:
            state = np_state if np_state is not None else np.random.get_state()
            (_, _), (key, pos) = mt_states(np_state=state)
            key_out, pos_out, draw = np.zeros(624, np.uint32), C.c_int32(-1), np.zeros(8, np.float64)
            st = self._lib.midas_sites_scan_resampled(*common, int(rand_reads), int(bool(replace_reads)), p(key), pos, p(key_out),
                                                      C.byref(pos_out), p(draw))
        elif _classes is not None:
            cls = None if _classes[0] is None else np.ascontiguousarray(_classes[0], dtype=np.uint8)
            assert cls is None or cls.shape[0] == N
            st = self._lib.midas_sites_scan_classes(*common, p(cls), int(_classes[1]))
        else:
            st = self._lib.midas_sites_scan(*common)
        self._check_bad(st, stats)
        if rand_reads:
            out.update(np_state=(state[0], key_out, pos_out.value) + tuple(state[3:]), n_resampled=int(stats[11]), n_drew=int(stats[12]),
                       raw_made=int(draw[0]), accepted_used=int(draw[1]), raw_consumed=int(draw[2]), draw_ms=draw[3:].tolist())
        n = int(stats[0])
        out.update(n_sites=n, n_kept=int(stats[1]), side_freq=int(stats[2]), side_depth=int(stats[3]), groups=int(stats[7]),
                   no_gene=int(stats[8]), group_rows=int(stats[9]), chunk_bytes=int(stats[10]), ms=ms.tolist())
        if seq is not None:
            out['seq'] = seq[:, :out['n_kept']]
        if dump:
            out.update(freq=out['freq'][:, :n], depthv=out['depthv'][:, :n], keep=out['keep'][:n], pooled=out['pooled'][:n])
        elif dump_keep:
            out['keep'] = out['keep'][:n]
        return out

    def sites_scan_classes(self, freq_text, depth_text, site_mask, site_class, n_classes: int, sample_col, mean_depth, site_depth: int,
                           site_ratio: float, allele_support: float, site_prev: float, site_maf: float, **kw):
        """midas_sites_scan_classes(): sites_scan's sums once per site class in one pass.  site_class uint8 [N] (None with
        n_classes 1: every site is class 0), n_classes 1 .. SITES_MAX_CLASSES; the other arguments and the result are sites_scan's
        (no SITES_SEQ, no rand_reads), with pi / snps / sites / depth [n_classes, chains, genes]: block c is sites_scan's for
        site_mask & (site_class == c) with the same retained sites.  n_kept, max_sites and no_gene count sites of every class."""
        assert not kw.get('rand_reads')
        return self.sites_scan(freq_text, depth_text, site_mask, sample_col, mean_depth, site_depth, site_ratio, allele_support, site_prev,
                               site_maf, _classes=(site_class, n_classes), **kw)

    def _strains_call(self, fn, freq_text, depth_text, n_parse, n_call, site_arrays, sample_col, min_freq, iparams, out):
        ft = np.ascontiguousarray(freq_text, dtype=np.uint8)
        dt = np.ascontiguousarray(depth_text, dtype=np.uint8)
        cols = np.ascontiguousarray(sample_col, dtype=np.int32)
        assert cols.shape[0] >= 1 and 0 <= n_call <= n_parse and all(a.shape[0] >= n_call for a in site_arrays)
        fp = np.array([min_freq, 0.0], np.float64)
        ip = np.array(list(iparams) + [0] * (8 - len(iparams)), np.int64)
        stats, ms = np.zeros(16, np.int64), np.zeros(8, np.float32)
        p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None
        st = fn(self._h, p(ft), ft.shape[0], p(dt), dt.shape[0], int(n_parse), int(n_call), *[p(a) for a in site_arrays], cols.shape[0],
                p(cols), p(fp), p(ip), p(out), p(stats), p(ms))
        self._check_bad(st, stats)
        return dict(n_sites=int(stats[0]), groups=int(stats[7]), side_freq=int(stats[2]), side_depth=int(stats[3]),
                    group_rows=int(stats[9]), chunk_bytes=int(stats[10]), ms=ms.tolist()), stats

    def sites_id_markers(self, freq_text, depth_text, minor_code, major_code, sample_col, min_freq: float, min_reads: int, allele_prev: int,
                         n_parse: int = None, group_rows: int = 0, chunk_bytes: int = 0):
        """midas_sites_id_markers(): strain_tracking.py id_markers over the text rows of the two matrices.  minor_code / major_code
        uint8 [n_call]: the site's alleles as indices into ALLELE_LETTERS (anything above 3: another string); rows up to n_parse
        (default n_call) are read and checked.  -> dict(rows int32 [markers, 7] = site row, allele, samples with depth, samples
        with A, T, C, G; n_sites, groups, side_freq, side_depth, ms [8]).  A row that cannot be read or called raises
        MidasSnpsError with .bad = (1 freq | 2 depth | 3 not finite | 4 minor letter | 5 major letter, data row, sample or -1)."""
        mi = np.ascontiguousarray(minor_code, dtype=np.uint8)
        ma = np.ascontiguousarray(major_code, dtype=np.uint8)
        n_call = int(mi.shape[0])
        assert ma.shape[0] == n_call
        rows = np.zeros((max(n_call, 1), 7), np.int32)
        out, stats = self._strains_call(self._lib.midas_sites_id_markers, freq_text, depth_text, n_call if n_parse is None else n_parse, n_call,
                                        [mi, ma], sample_col, float(min_freq), [int(min_reads), int(allele_prev), group_rows, chunk_bytes, n_call], rows)
        out['rows'] = rows[:int(stats[1])]
        return out

    def sites_track_markers(self, freq_text, depth_text, site_which, sample_col, min_freq: float, min_reads: int, n_parse: int = None,
                            group_rows: int = 0, chunk_bytes: int = 0, pair_blocks: int = 0):
        """midas_sites_track_markers(): strain_tracking.py track_markers.  site_which uint8 [n_call]: 0 no marker, 1 the marker is the
        site's major, 2 its minor allele.  -> dict(both int64 [S, S], filled for i <= j: sites whose marker both samples have (the
        diagonal: the sample's own count); n_matched, word_pairs, pair_runs / pair_steps = the most word runs a launch of the pair
        kernel had and the most staging steps a run had, n_sites, groups, ms [8]); errors as sites_id_markers.  pair_blocks: the
        workgroups the pair kernel aims at when it cuts the words into runs (0: 1024); the output does not depend on it."""
        which = np.ascontiguousarray(site_which, dtype=np.uint8)
        n_call = int(which.shape[0])
        S = int(np.asarray(sample_col).shape[0])
        both = np.zeros((S, S), np.int64)
        out, stats = self._strains_call(self._lib.midas_sites_track_markers, freq_text, depth_text, n_call if n_parse is None else n_parse, n_call,
                                        [which], sample_col, float(min_freq), [int(min_reads), 0, group_rows, chunk_bytes, 0, int(pair_blocks)], both)
        out.update(both=both, n_matched=int(stats[1]), word_pairs=int(stats[8]), pair_runs=int(stats[11]), pair_steps=int(stats[12]))
        return out

    def sites_consensus_pairs(self, freq_text, depth_text, site_mask, sample_col, mean_depth, site_depth: int, site_ratio: float,
                              allele_support: float, site_prev: float, site_maf: float, max_sites: int = -1, flags: int = 0,
                              group_rows: int = 0, chunk_bytes: int = 0, pair_blocks: int = 0):
        """midas_sites_consensus_pairs(): the sites call_consensus.py retains (sites_scan's arguments under SITES_SEQ; of flags
        SITES_MASK_ONLY alone counts), every (site, sample) call as two bit planes, and the pair counts over them.  -> dict(both /
        diff int64 [S, S], filled for i <= j: sites called in both samples / those where the two calls are the minor and the major
        allele; n_sites, n_kept, side_freq, side_depth, groups, word_pairs, pair_runs, pair_steps, sample_limit, ms [8]).  A
        malformed row raises MidasSnpsError with .bad as sites_scan; more samples than the pair matrices fit the free device
        memory for raises it with .limit = that number.  pair_blocks as sites_track_markers: the output does not depend on it."""
        ft = np.ascontiguousarray(freq_text, dtype=np.uint8)
        dt = np.ascontiguousarray(depth_text, dtype=np.uint8)
        mask = np.ascontiguousarray(site_mask, dtype=np.uint8)
        cols = np.ascontiguousarray(sample_col, dtype=np.int32)
        mean = np.ascontiguousarray(mean_depth, dtype=np.float64)
        S = int(cols.shape[0])
        assert mean.shape[0] == S and S >= 1
        fp = np.array([site_ratio, allele_support, site_prev, site_maf, 0.0], np.float64)
        ip = np.array([site_depth, max_sites, flags & SITES_MASK_ONLY, 0, group_rows, chunk_bytes, pair_blocks, 0], np.int64)
        both, diff = np.zeros((S, S), np.int64), np.zeros((S, S), np.int64)
        stats, ms = np.zeros(16, np.int64), np.zeros(8, np.float32)
        p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None
        st = self._lib.midas_sites_consensus_pairs(self._h, p(ft), ft.shape[0], p(dt), dt.shape[0], int(mask.shape[0]), p(mask), S, p(cols),
                                                   p(mean), p(fp), p(ip), p(both), p(diff), p(stats), p(ms))
        try:
            self._check_bad(st, stats)
        except MidasSnpsError as e:
            e.limit = int(stats[13]) if st == ERR_OUT_OF_MEMORY and stats[13] < S else None
            raise
        return dict(both=both, diff=diff, n_sites=int(stats[0]), n_kept=int(stats[1]), side_freq=int(stats[2]), side_depth=int(stats[3]),
                    groups=int(stats[7]), word_pairs=int(stats[8]), group_rows=int(stats[9]), chunk_bytes=int(stats[10]),
                    pair_runs=int(stats[11]), pair_steps=int(stats[12]), sample_limit=int(stats[13]), ms=ms.tolist())

    def sites_pair_diversity(self, freq_text, depth_text, site_mask, sample_col, mean_depth, site_depth: int, site_ratio: float,
                             allele_support: float, site_prev: float, site_maf: float, snp_maf: float = 0.01, max_sites: int = -1,
                             flags: int = 0, group_rows: int = 0, chunk_bytes: int = 0, pair_form: int = 0):
        """midas_sites_pair_diversity(): for every pair i < j of the samples what sites_scan gives under SITES_SUMS | SITES_POOLED
        with those two alone, and the sums over the sites both are kept at (sites_scan's arguments; of flags SITES_WEIGHT and
        SITES_ROUND count; max_sites is every pair's own).  -> dict(sites / snps / shared int64 [S, S], pi / w1 / w2 / x f64
        [S, S], filled above the diagonal; n_sites, n_masked, side_freq, side_depth, groups, pair_sites, pair_form (1 | 4 pairs a
        lane a side), tiles, sample_limit, ms [8]).  Errors as sites_consensus_pairs: .bad for a row, .limit for too many samples.
        pair_form 2 runs the 4 x 4 kernel (0, 1: one pair a lane, the faster one on an MI355X): the output does not depend on it."""
        ft = np.ascontiguousarray(freq_text, dtype=np.uint8)
        dt = np.ascontiguousarray(depth_text, dtype=np.uint8)
        mask = np.ascontiguousarray(site_mask, dtype=np.uint8)
        cols = np.ascontiguousarray(sample_col, dtype=np.int32)
        mean = np.ascontiguousarray(mean_depth, dtype=np.float64)
        S = int(cols.shape[0])
        assert mean.shape[0] == S
        fp = np.array([site_ratio, allele_support, site_prev, site_maf, snp_maf], np.float64)
        ip = np.array([site_depth, max_sites, flags & (SITES_WEIGHT | SITES_ROUND), 0, group_rows, chunk_bytes, pair_form, 0], np.int64)
        out = {k: np.zeros((S, S), np.int64) for k in ('sites', 'snps', 'shared')}
        out.update({k: np.zeros((S, S), np.float64) for k in ('pi', 'w1', 'w2', 'x')})
        stats, ms = np.zeros(16, np.int64), np.zeros(8, np.float32)
        p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None
        st = self._lib.midas_sites_pair_diversity(self._h, p(ft), ft.shape[0], p(dt), dt.shape[0], int(mask.shape[0]), p(mask), S, p(cols),
                                                  p(mean), p(fp), p(ip), *[p(out[k]) for k in ('sites', 'snps', 'shared', 'pi', 'w1', 'w2', 'x')],
                                                  p(stats), p(ms))
        try:
            self._check_bad(st, stats)
        except MidasSnpsError as e:
            e.limit = int(stats[13]) if st == ERR_OUT_OF_MEMORY and stats[13] < S else None
            raise
        out.update(n_sites=int(stats[0]), n_masked=int(stats[1]), side_freq=int(stats[2]), side_depth=int(stats[3]), groups=int(stats[7]),
                   pair_sites=int(stats[8]), group_rows=int(stats[9]), chunk_bytes=int(stats[10]), pair_form=int(stats[11]),
                   tiles=int(stats[12]), sample_limit=int(stats[13]), ms=ms.tolist())
        return out

    def sites_ld(self, freq_text, depth_text, site_mask, sample_col, mean_depth, site_key, site_gene, site_depth: int, site_ratio: float,
                 allele_support: float, site_prev: float, site_maf: float, max_dist: int = 1000, bin_width: int = 10, min_samples: int = 4,
                 max_sites: int = -1, flags: int = 0, group_rows: int = 0, chunk_bytes: int = 0, anchor_chunk: int = 0):
        """midas_sites_ld(): linkage disequilibrium between the sites call_consensus.py retains (sites_consensus_pairs' arguments;
        of flags SITES_MASK_ONLY and SITES_LD_SAME_GENE count), by distance bin.  site_key int64 [n]: contig index * 2^40 +
        ref_pos, strictly ascending over the rows of the mask; site_gene int32 [n] or None.  -> dict(window / pairs int64
        [n_bins] = pairs of sites / informative ones, sum_r2 / sum_d2 / sum_het f64 [n_bins]; n_sites, n_kept, side_freq,
        side_depth, groups, pairs_visited, group_rows, chunk_bytes, anchor_chunks, anchor_chunk, site_limit, ms [8]).  The
        arithmetic is the contract in include/midas_snps.h: the output depends on neither group_rows, chunk_bytes nor
        anchor_chunk.  A malformed row raises MidasSnpsError with .bad as sites_scan; more rows in the mask than the planes fit
        the free device memory for raises it with .limit = that number."""
        ft = np.ascontiguousarray(freq_text, dtype=np.uint8)
        dt = np.ascontiguousarray(depth_text, dtype=np.uint8)
        mask = np.ascontiguousarray(site_mask, dtype=np.uint8)
        cols = np.ascontiguousarray(sample_col, dtype=np.int32)
        mean = np.ascontiguousarray(mean_depth, dtype=np.float64)
        key = np.ascontiguousarray(site_key, dtype=np.int64)
        gene = None if site_gene is None else np.ascontiguousarray(site_gene, dtype=np.int32)
        S, n = int(cols.shape[0]), int(mask.shape[0])
        assert mean.shape[0] == S and S >= 1 and key.shape[0] == n and (gene is None or gene.shape[0] == n)
        n_bins = -(-int(max_dist) // int(bin_width)) if max_dist >= 1 and bin_width >= 1 else 1
        fp = np.array([site_ratio, allele_support, site_prev, site_maf, 0.0], np.float64)
        ip = np.array([site_depth, max_sites, flags & (SITES_MASK_ONLY | SITES_LD_SAME_GENE), min_samples, group_rows, chunk_bytes, anchor_chunk, 0],
                      np.int64)
        out = {k: np.zeros(n_bins, np.int64) for k in ('window', 'pairs')}
        out.update({k: np.zeros(n_bins, np.float64) for k in ('sum_r2', 'sum_d2', 'sum_het')})
        stats, ms = np.zeros(16, np.int64), np.zeros(8, np.float32)
        p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None
        st = self._lib.midas_sites_ld(self._h, p(ft), ft.shape[0], p(dt), dt.shape[0], n, p(mask), S, p(cols), p(mean), p(fp), p(ip), p(key),
                                      p(gene), int(max_dist), int(bin_width), *[p(out[k]) for k in ('window', 'pairs', 'sum_r2', 'sum_d2', 'sum_het')],
                                      p(stats), p(ms))
        try:
            self._check_bad(st, stats)
        except MidasSnpsError as e:
            e.limit = int(stats[13]) if st == ERR_OUT_OF_MEMORY and stats[13] > 0 else None
            raise
        out.update(n_sites=int(stats[0]), n_kept=int(stats[1]), side_freq=int(stats[2]), side_depth=int(stats[3]), groups=int(stats[7]),
                   pairs_visited=int(stats[8]), group_rows=int(stats[9]), chunk_bytes=int(stats[10]), anchor_chunks=int(stats[11]),
                   anchor_chunk=int(stats[12]), site_limit=int(stats[13]), ms=ms.tolist())
        return out

    def nj_tree(self, dist):
        """midas_nj_tree(): neighbour joining over a symmetric matrix of finite doubles [n, n], n >= 3, on the device; the
        arithmetic is the contract in include/midas_snps.h.  -> dict(join int32 [n - 3, 2] = the slots (a, b) joined at every
        step (slot a holds the new node), len f64 [n - 3, 2] = their branch lengths, last int32 [3] / last_len f64 [3] = the three
        slots left and their lengths, sample_limit, ms [8] = upload, steps, download).  A matrix the free device memory does not
        hold raises MidasSnpsError with .limit = the largest n it holds."""
        d = np.ascontiguousarray(dist, dtype=np.float64)
        n = int(d.shape[0])
        assert d.shape == (n, n)
        join, length = np.zeros((max(n - 3, 0), 2), np.int32), np.zeros((max(n - 3, 0), 2), np.float64)
        last, last_len = np.zeros(3, np.int32), np.zeros(3, np.float64)
        stats, ms = np.zeros(16, np.int64), np.zeros(8, np.float32)
        p = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None
        st = self._lib.midas_nj_tree(self._h, n, p(d), p(join), p(length), p(last), p(last_len), p(stats), p(ms))
        if st != 0:
            try:
                self._check(st)
            except MidasSnpsError as e:
                e.limit = int(stats[0]) if st == ERR_OUT_OF_MEMORY and 0 < stats[0] < n else None
                raise
        return dict(join=join, len=length, last=last, last_len=last_len, sample_limit=int(stats[0]), ms=ms.tolist())

    def genes_compare(self, text, n_rows: int, n_samples: int, n_columns: int, dtype: str = 'presabs', distance: str = 'jaccard',
                      cutoff: float = 0.35, group_rows: int = 0, chunk_bytes: int = 0, pair_blocks: int = 0, dump: bool = False):
        """midas_genes_compare(): compare_genes.py over the text rows of genes_copynum.txt, the first n_samples of n_columns sample
        columns, rows [0, n_rows).  -> dict(dtype, distance, n_samples, n_rows read, col_float uint8 [S], groups, steps, tiles,
        group_rows, chunk_bytes, ms [8]; presabs: count int64 [S, S]; copynum: both, either and (euclidean / manhattan) dist f64
        [S, S], all filled for i <= j; with dump: cells f64 [S, n_rows]).  A malformed row raises MidasSnpsError with
        .bad = (1 width | 2 cell, data row, sample column or -1)."""
        tx = np.ascontiguousarray(text, dtype=np.uint8)
        S, N = int(n_samples), int(n_rows)
        copynum = dtype == 'copynum'
        kd = GENES_DISTANCES[distance]
        count = None if copynum else np.zeros((S, S), np.int64)
        both = np.zeros((S, S), np.float64) if copynum else None
        either = np.zeros((S, S), np.float64) if copynum else None
        dist = np.zeros((S, S), np.float64) if copynum and kd else None
        col_float = np.zeros(S, np.uint8)
        cells = np.zeros((S, max(N, 1)), np.float64) if dump else None
        ip = np.array([group_rows, chunk_bytes, pair_blocks, 0], np.int64)
        stats, ms = np.zeros(16, np.int64), np.zeros(8, np.float32)
        p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None
        st = self._lib.midas_genes_compare(self._h, p(tx), tx.shape[0], N, S, int(n_columns), GENES_DTYPES[dtype], kd, float(cutoff), p(ip),
                                           p(count), p(both), p(either), p(dist), p(col_float), p(cells), p(stats), p(ms))
        self._check_bad(st, stats)
        n = int(stats[0])
        out = dict(dtype=dtype, distance=distance, n_samples=S, n_rows=n, col_float=col_float, groups=int(stats[7]), steps=int(stats[8]),
                   tiles=int(stats[11]), group_rows=int(stats[9]), chunk_bytes=int(stats[10]), ms=ms.tolist(), count=count, both=both,
                   either=either, dist=dist)
        if dump:
            out['cells'] = cells[:, :n]
        return out

    def genes_linkage(self, text, n_rows: int, n_samples: int, n_columns: int, need, cutoff: float = 0.35, min_present: int = 2,
                      min_absent: int = 2, max_pairs: int = 1 << 26, group_rows: int = 0, chunk_bytes: int = 0, pair_form: int = 0,
                      pair_out=None):
        """midas_genes_linkage(): gene_linkage.py over the text rows of genes_copynum.txt, the first n_samples of n_columns sample
        columns, rows [0, n_rows).  need: int32 [n_samples + 1], the fewest shared samples that link a pair at every size of the
        union.  -> dict(n_rows read, n_samples, n_kept K, count, row_of_slot, label int32 [K], pair_a, pair_b, pair_both int32
        [linked], visited, linked, label_rounds, groups, group_rows, chunk_bytes, form, strips, ms [8]).  More than max_pairs
        linked pairs raises MidasSnpsError (ERR_OUT_OF_MEMORY) with .linked = the exact total; a malformed row raises it with
        .bad as genes_compare.  pair_out (tests): three int32 arrays of max_pairs entries to receive the pairs."""
        tx = np.ascontiguousarray(text, dtype=np.uint8)
        S, N, cap = int(n_samples), int(n_rows), int(max_pairs)
        nd = np.ascontiguousarray(need, dtype=np.int32)
        if nd.shape != (S + 1,):
            raise MidasSnpsError(ERR_INVALID_ARG, "need must hold n_samples + 1 entries")
        count, row, label = np.zeros(N, np.int32), np.zeros(N, np.int32), np.zeros(N, np.int32)
        pa, pb, pc = pair_out if pair_out is not None else (np.empty(cap, np.int32), np.empty(cap, np.int32), np.empty(cap, np.int32))
        ip = np.array([group_rows, chunk_bytes, min_present, min_absent, pair_form, 0, 0, 0], np.int64)
        stats, ms = np.zeros(16, np.int64), np.zeros(8, np.float32)
        p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None
        st = self._lib.midas_genes_linkage(self._h, p(tx), tx.shape[0], N, S, int(n_columns), float(cutoff), p(ip), p(nd), cap, p(count),
                                           p(row), p(label), p(pa), p(pb), p(pc), p(stats), p(ms))
        try:
            self._check_bad(st, stats)
        except MidasSnpsError as e:
            e.linked = int(stats[11]) if st == ERR_OUT_OF_MEMORY and stats[11] > cap else None
            raise
        K, n = int(stats[1]), int(stats[11])
        return dict(n_rows=int(stats[0]), n_samples=S, n_kept=K, count=count[:K], row_of_slot=row[:K], label=label[:K],
                    pair_a=pa[:n].copy(), pair_b=pb[:n].copy(), pair_both=pc[:n].copy(), visited=int(stats[8]), linked=n,
                    label_rounds=int(stats[12]), groups=int(stats[7]), group_rows=int(stats[9]), chunk_bytes=int(stats[10]),
                    form=int(stats[13]), strips=int(stats[14]), ms=ms.tolist())

    def genes_assoc(self, text, n_rows: int, n_samples: int, n_columns: int, use, case, planes, cutoff: float = 0.35,
                    dtype: str = 'presabs', min_present: int = 1, min_absent: int = 0, group_rows: int = 0, chunk_bytes: int = 0,
                    form: int = 1, products: bool = False):
        """midas_genes_assoc(): gene_assoc.py over the text rows of genes_copynum.txt, the first n_samples of n_columns sample
        columns, rows [0, n_rows).  use, case: uint64 [ceil(n_samples / 64)], bit s: column s takes part / is a case; planes:
        uint64 [P, ceil(n_samples / 64)], the relabellings (P may be 0).  -> dict(n_rows read, n_samples, n_used N, n_case n1,
        n_perms P, dtype, n_kept K, row_of_slot, count, count_case int32 [K], w, ties int64 [K], exceed uint32 [K], groups,
        group_rows, chunk_bytes, form, in_lds, ms [8]; with products (tests): products int32 [K, P]).  A malformed row raises
        MidasSnpsError with .bad as genes_compare."""
        tx = np.ascontiguousarray(text, dtype=np.uint8)
        S, N = int(n_samples), int(n_rows)
        W = (S + 63) // 64
        us, cs = np.ascontiguousarray(use, dtype=np.uint64), np.ascontiguousarray(case, dtype=np.uint64)
        pl = np.ascontiguousarray(planes, dtype=np.uint64).reshape(-1, W)
        if us.shape != (W,) or cs.shape != (W,):
            raise MidasSnpsError(ERR_INVALID_ARG, "use and case must hold ceil(n_samples / 64) words")
        P = pl.shape[0]
        row, count, ccase = np.zeros(N, np.int32), np.zeros(N, np.int32), np.zeros(N, np.int32)
        w, ties, exceed = np.zeros(N, np.int64), np.zeros(N, np.int64), np.zeros(N, np.uint32)
        prod = np.zeros(min(N * P, 1 << 24), np.int32) if products else None
        ip = np.array([group_rows, chunk_bytes, min_present, min_absent, GENES_DTYPES[dtype], form, 0, 0], np.int64)
        stats, ms = np.zeros(16, np.int64), np.zeros(8, np.float32)
        p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None
        st = self._lib.midas_genes_assoc(self._h, p(tx), tx.shape[0], N, S, int(n_columns), us.ctypes.data_as(C.c_void_p),
                                         cs.ctypes.data_as(C.c_void_p), p(pl), P, float(cutoff), p(ip), p(row), p(count), p(ccase), p(w),
                                         p(ties), p(exceed), p(prod), p(stats), p(ms))
        self._check_bad(st, stats)
        K = int(stats[1])
        out = dict(n_rows=int(stats[0]), n_samples=S, n_used=int(stats[11]), n_case=int(stats[12]), n_perms=P, dtype=dtype, n_kept=K,
                   row_of_slot=row[:K], count=count[:K], count_case=ccase[:K], w=w[:K], ties=ties[:K], exceed=exceed[:K],
                   groups=int(stats[7]), group_rows=int(stats[9]), chunk_bytes=int(stats[10]), form=int(stats[13]), in_lds=int(stats[8]),
                   ms=ms.tolist())
        if products:
            out['products'] = prod[:K * P].reshape(K, P).copy()
        return out

    def species_classify(self, text, gene_names, gene_species, gene_marker, n_species: int, marker_cutoff, aln_cov: float,
                         chunk_bytes: int = 0, hash_bits: int = 0, dump: bool = False):
        """midas_species_classify(): the lines of alignments.m8 (bytes or a uint8 array) against the marker genes gene_names
        (list of bytes) with their species / marker-family indices.  -> dict(lines, passing, unique, ambiguous, uniq_reads and
        uniq_aln int64 [n_species], indptr int64 [ambiguous + 1], hit_species and hit_aln int32, side_cells, chunks, chunk_bytes,
        ms [8]; with dump: pid, score f64 and aln, qlen, species, marker int32 and passed uint8 per line).  A bad line raises
        MidasSnpsError with .bad = (reason, 1-based line), the earliest one of the file."""
        tx = np.frombuffer(text, np.uint8) if isinstance(text, (bytes, bytearray, memoryview)) else np.ascontiguousarray(text, dtype=np.uint8)
        names = np.frombuffer(b''.join(gene_names), np.uint8)
        off = np.zeros(len(gene_names) + 1, np.int64)
        np.cumsum([len(g) for g in gene_names], out=off[1:])
        gs, gm = np.ascontiguousarray(gene_species, np.int32), np.ascontiguousarray(gene_marker, np.int32)
        cut = np.ascontiguousarray(marker_cutoff, np.float64)
        S = int(n_species)
        ur, ua = np.zeros(S, np.int64), np.zeros(S, np.int64)
        ip = np.array([chunk_bytes, hash_bits, 1 if dump else 0, 0], np.int64)
        stats, ms = np.zeros(16, np.int64), np.zeros(8, np.float32)
        res = C.c_void_p()
        p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None
        st = self._lib.midas_species_classify(self._h, p(tx), tx.size, len(gene_names), p(names), p(off), p(gs), p(gm), S, cut.size, p(cut),
                                              float(aln_cov), p(ip), p(ur), p(ua), p(stats), p(ms), C.byref(res))
        if st != 0:
            try:
                self._check(st)
            except MidasSnpsError as e:
                e.bad = (int(stats[4]), int(stats[5])) if stats[4] else None
                raise
        try:
            n, n_amb, n_hits = int(stats[0]), int(stats[3]), int(stats[9])
            indptr, hs, ha = np.zeros(n_amb + 1, np.int64), np.zeros(n_hits, np.int32), np.zeros(n_hits, np.int32)
            self._check(self._lib.midas_species_result_columns(res, p(indptr), p(hs), p(ha)))
            out = dict(lines=n, passing=int(stats[1]), unique=int(stats[2]), ambiguous=n_amb, uniq_reads=ur, uniq_aln=ua, indptr=indptr,
                       hit_species=hs, hit_aln=ha, side_cells=int(stats[6]), chunks=int(stats[7]), chunk_bytes=int(stats[8]), ms=ms.tolist())
            if dump:
                cols = dict(pid=np.zeros(n, np.float64), score=np.zeros(n, np.float64), aln=np.zeros(n, np.int32), qlen=np.zeros(n, np.int32),
                            species=np.zeros(n, np.int32), marker=np.zeros(n, np.int32), passed=np.zeros(n, np.uint8))
                self._check(self._lib.midas_species_result_lines(res, *[p(cols[k]) for k in ('pid', 'score', 'aln', 'qlen', 'species', 'marker', 'passed')]))
                out.update(cols)
        finally:
            self._lib.midas_species_result_close(res)
        return out

    def species_merge(self, profile_paths, species_ids, sample_depth: float = 1.0, chunk_bytes: int = 0, lds_bound: int = 0, threads: int = 0):
        """midas_species_merge(): the samples' species_profile.txt files (paths, in sample order) against the species ids of
        species_info.txt (distinct, in row order).  -> SpeciesMerge: coverage, abundance fp64 and reads int64 [species][sample]; per
        species mean_coverage, median_coverage, mean_abundance, median_abundance and rounded[...] of each, prevalence, order (the
        species of every row of species_prevalence.txt); lines, groups, chunk_bytes, side_cells, lds_rows, ms [8]; .write(outdir,
        sample_ids) writes the four files.  A bad profile raises MidasSnpsError naming file, line and species or column, with
        .bad = (reason, sample, 1-based line): the earliest one in the order of samples, then lines."""
        paths = [os.fsencode(q) for q in profile_paths]
        ids = [s.encode() if isinstance(s, str) else bytes(s) for s in species_ids]
        arr = (C.c_char_p * len(paths))(*paths)
        names = np.frombuffer(b''.join(ids), np.uint8)
        off = np.zeros(len(ids) + 1, np.int64)
        np.cumsum([len(g) for g in ids], out=off[1:])
        if names.size == 0:
            names = np.zeros(1, np.uint8)
        ip = np.array([chunk_bytes, lds_bound, threads, 0], np.int64)
        stats, ms = np.zeros(16, np.int64), np.zeros(8, np.float32)
        res = C.c_void_p()
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        st = self._lib.midas_species_merge(self._h, len(paths), C.cast(arr, C.c_void_p), len(ids), p(names), p(off), float(sample_depth), p(ip), p(stats),
                                           p(ms), C.byref(res))
        self._check_bad(st, stats)
        return SpeciesMerge(self._lib, res, len(ids), len(paths), stats, ms)

    def batch(self, contigs: ContigTable, reads: ReadsSoA) -> "Batch":
        return Batch(self, contigs, reads)


class SpeciesMerge:
    """What Context.species_merge returns: the matrices and the per-species numbers as arrays, and the writer of the four files."""

    def __init__(self, lib, handle, n_species, n_samples, stats, ms):
        self._lib, self._h = lib, handle
        R, S = n_species, n_samples
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        try:
            self.coverage, self.abundance, self.reads = np.zeros((R, S), np.float64), np.zeros((R, S), np.float64), np.zeros((R, S), np.int64)
            st8, self.prevalence, self.order = np.zeros((8, R), np.float64), np.zeros(R, np.int64), np.zeros(R, np.int32)
            for st in (lib.midas_species_merge_result_matrices(handle, p(self.coverage), p(self.abundance), p(self.reads)),
                       lib.midas_species_merge_result_stats(handle, p(st8), p(self.prevalence), p(self.order))):
                if st != 0:
                    raise MidasSnpsError(st, "midas_species_merge_result: " + lib.midas_snps_status_string(st).decode())
        except Exception:
            self.close()
            raise
        self.rounded = {}
        for k, name in enumerate(SPECIES_MERGE_STATS):
            setattr(self, name, st8[k])
            self.rounded[name] = st8[4 + k]
        self.lines, self.groups, self.chunk_bytes, self.side_cells = int(stats[0]), int(stats[1]), int(stats[2]), int(stats[3])
        self.lds_rows, self.text_bytes, self.ms = bool(stats[8]), int(stats[11]), ms.tolist()

    def write(self, outdir, sample_ids, threads: int = 0):
        """relative_abundance.txt, coverage.txt, count_reads.txt and species_prevalence.txt into outdir."""
        err = C.create_string_buffer(1024)
        header = '\t'.join(['species_id'] + list(sample_ids)) + '\n'
        st = self._lib.midas_species_merge_result_write(self._h, os.fsencode(outdir), header.encode(), threads, err)
        if st != 0:
            raise MidasSnpsError(st, err.value.decode() or "midas_species_merge_result_write failed")

    def close(self):
        if self._h:
            self._lib.midas_species_merge_result_close(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        self.close()


class Comm:
    """An RCCL communicator of the ranks' contexts (comm.cpp): the all-gather of the summary rows over xGMI and the genes
    path's all-to-all, with no process group behind them.  midas_amd/dist.py makes one per job (the id travels through a file)."""

    def __init__(self, ctx: "Context", id128: bytes, rank: int, world: int):
        self._lib = ctx._lib
        self.rank, self.world = int(rank), int(world)
        h = C.c_void_p()
        err = C.create_string_buffer(256)
        buf = C.create_string_buffer(bytes(id128), 128)
        st = self._lib.midas_comm_create(ctx._h, C.cast(buf, C.c_void_p), self.rank, self.world, C.byref(h), err)
        if st != 0:
            raise MidasSnpsError(st, err.value.decode() or "midas_comm_create failed")
        self._h = h
        self._ctx = ctx          # (the communicator runs on the context's stream: keep it alive)

    @staticmethod
    def unique_id() -> bytes:
        lib = load_library()
        out, err = C.create_string_buffer(128), C.create_string_buffer(256)
        st = lib.midas_comm_unique_id(C.cast(out, C.c_void_p), err)
        if st != 0:
            raise MidasSnpsError(st, err.value.decode() or "midas_comm_unique_id failed")
        return out.raw

    @staticmethod
    def probe() -> int:
        """RCCL's version when this process can use it at all (midas_comm_probe); raises MidasSnpsError when it cannot."""
        lib = load_library()
        v, err = C.c_int32(0), C.create_string_buffer(256)
        st = lib.midas_comm_probe(C.byref(v), err)
        if st != 0:
            raise MidasSnpsError(st, err.value.decode() or "midas_comm_probe failed")
        return int(v.value)

    @staticmethod
    def device_key(ctx: "Context") -> str:
        out = C.create_string_buffer(64)
        ctx._check(ctx._lib.midas_comm_device_key(ctx._h, out))
        return out.value.decode()

    def close(self):
        if getattr(self, '_h', None):
            self._lib.midas_comm_destroy(self._h)
            self._h = None

    __del__ = close

    def all_gather(self, data: bytes):
        """every rank's `data` (the same length everywhere), by rank"""
        n = len(data)
        out, err = C.create_string_buffer(max(1, n * self.world)), C.create_string_buffer(256)
        src = C.create_string_buffer(bytes(data), max(1, n))
        st = self._lib.midas_comm_all_gather(self._h, C.cast(src, C.c_void_p), C.cast(out, C.c_void_p), n, err)
        if st != 0:
            raise MidasSnpsError(st, err.value.decode() or "midas_comm_all_gather failed")
        raw = out.raw
        return [raw[r * n:(r + 1) * n] for r in range(self.world)]

    def all_to_all_v(self, parts, recv_bytes):
        """parts[r]: the bytes for rank r; recv_bytes[r]: how many come from rank r -> the bytes received, by source rank"""
        send = b"".join(bytes(p) for p in parts)
        sb = np.array([len(p) for p in parts], np.int64)
        rb = np.array([int(x) for x in recv_bytes], np.int64)
        out, err = C.create_string_buffer(max(1, int(rb.sum()))), C.create_string_buffer(256)
        src = C.create_string_buffer(send, max(1, len(send)))
        st = self._lib.midas_comm_all_to_all_v(self._h, C.cast(src, C.c_void_p), sb.ctypes.data_as(C.c_void_p), C.cast(out, C.c_void_p),
                                               rb.ctypes.data_as(C.c_void_p), err)
        if st != 0:
            raise MidasSnpsError(st, err.value.decode() or "midas_comm_all_to_all_v failed")
        raw, got, at = out.raw, [], 0
        for n in rb:
            got.append(raw[at:at + int(n)])
            at += int(n)
        return got


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
        p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
        self.ctx._check(self._lib.midas_snps_batch_fetch(self._h, p(oc), p(oa), p(os_)))
        return oc, oa, os_

    def write_part(self, path: str, contig_index, ref_ids, header: bool = True, gz_level: int = 4, threads: int = 0):
        """Rows of the contigs contig_index (indices into the batch's contig table, output order) straight from the device
        results into a gzip table or part of one (midas_snps_batch_write_part)."""
        n = len(contig_index)
        idx = np.ascontiguousarray(contig_index, dtype=np.int32)
        ids = (C.c_char_p * max(n, 1))(*[r.encode() for r in ref_ids])
        self.ctx._check(self._lib.midas_snps_batch_write_part(self._h, path.encode(), 1 if header else 0, n,
                                                              idx.ctypes.data_as(C.c_void_p), ids, int(gz_level), int(threads)))

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
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        self.ctx._check(self._lib.midas_snps_batch_fetch_packed(self._h, p(rec), p(blob), p(orig), p(key), C.byref(n), C.byref(nb)))
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
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        self.ctx._check(self._lib.midas_snps_batch_fetch_index(self._h, p(tb), p(te), p(facts), p(out3), p(flag), p(ok), C.byref(n_ok)))
        f = dict(zip(INDEX_FACTS, (int(x) for x in facts)))
        return dict(tbegin=tb[:nt], tend=te[:nt], facts=f, outliers=out3[:min(f['n_outliers_listed'], cap)].copy(), tile_flag=flag[:nt],
                    chunk_ok=ok[:n_ok.value].copy())

    def stats_to_device(self, dst_device_ptr: int):
        """Enqueue a D2D copy of the [n_species,4] int64 counters into caller-owned device memory."""
        self.ctx._check(self._lib.midas_snps_batch_stats_to_device(self._h, C.c_void_p(dst_device_ptr)))
