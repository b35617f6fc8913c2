"""run_species.py (the m8 classify step and the serial assignment) and merge_species.py (the species profiles merged)."""

from __future__ import annotations

import ctypes as C
import os

import numpy as np

from .core import MidasSnpsError, P, addr, cstr, f64, host_call, i32, i64, load_library, mt_states, ptr, register, vp

# listed by themselves (SPECIES_SYMBOLS)
register('species', {
    'midas_species_classify': (i32, [vp, vp, i64, i32, vp, vp, vp, vp, i32, i32, vp, f64, vp, vp, vp, vp, vp, P(vp)]),
    'midas_species_result_columns': (i32, [vp, vp, vp, vp]),
    'midas_species_result_lines': (i32, [vp] * 8),
    'midas_species_result_close': (None, [vp]),
    'midas_species_assign': (i32, [i64, vp, vp, vp, i32, vp, i32, vp, i32, vp, vp, vp]),
    'midas_species_parse_number': (i32, [i32, cstr, i64, vp, P(i32)]),
})
# listed by themselves (SPECIES_MERGE_SYMBOLS)
register('species_merge', {
    'midas_species_merge': (i32, [vp, i32, vp, i32, vp, vp, f64, vp, vp, vp, P(vp)]),
    'midas_species_merge_result_matrices': (i32, [vp, vp, vp, vp]),
    'midas_species_merge_result_stats': (i32, [vp, vp, vp, vp]),
    'midas_species_merge_result_write': (i32, [vp, cstr, cstr, i32, cstr]),
    'midas_species_merge_result_close': (None, [vp]),
})

SPECIES_PHASES = ('upload', 'line index', 'fields', 'lookup', 'filter + sort + group', 'best hits', 'download')
SPECIES_REASONS = {1: 'fields', 2: 'target', 3: 'qlen', 4: 'aln', 5: 'number', 6: 'cutoff', 7: 'score nan'}
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
    st = lib.midas_species_assign(ip.size - 1, ptr(ip), ptr(hs), ptr(ha), r.size, ptr(pw), pp, ptr(nw), npos, ptr(r), ptr(a), ptr(draws))
    if st != 0:
        raise MidasSnpsError(st, "midas_species_assign: " + lib.midas_snps_status_string(st).decode())
    return r, a, (int(draws[0]), int(draws[1]))


def _name_blob(names):
    """A list of byte strings as (all of them back to back uint8, offsets int64 [n + 1])."""
    off = np.zeros(len(names) + 1, np.int64)
    np.cumsum([len(g) for g in names], out=off[1:])
    return np.frombuffer(b''.join(names), np.uint8), off


class SpeciesMerge:
    """What Context.species_merge returns: the matrices and the per-species numbers as arrays, and the writer of the four files."""

    def __init__(self, lib, handle, n_species, n_samples, stats, ms):
        self._lib, self._h = lib, handle
        R, S = n_species, n_samples
        try:
            self.coverage, self.abundance, self.reads = np.zeros((R, S), np.float64), np.zeros((R, S), np.float64), np.zeros((R, S), np.int64)
            st8, self.prevalence, self.order = np.zeros((8, R), np.float64), np.zeros(R, np.int64), np.zeros(R, np.int32)
            # (addr: a merge of no species, or of no samples, still hands over its empty matrices)
            for st in (lib.midas_species_merge_result_matrices(handle, addr(self.coverage), addr(self.abundance), addr(self.reads)),
                       lib.midas_species_merge_result_stats(handle, addr(st8), addr(self.prevalence), addr(self.order))):
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
        header = '\t'.join(['species_id'] + list(sample_ids)) + '\n'
        host_call(self._lib.midas_species_merge_result_write, self._h, os.fsencode(outdir), header.encode(), threads, wide=True,
                  what="midas_species_merge_result_write")

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


class _SpeciesCalls:
    """Context's species commands."""

    def species_classify(self, text, gene_names, gene_species, gene_marker, n_species: int, marker_cutoff, aln_cov: float,
                         chunk_bytes: int = 0, hash_bits: int = 0, dump: bool = False):
        """midas_species_classify(): the lines of alignments.m8 (bytes or a uint8 array) against the marker genes gene_names
        (list of bytes) with their species / marker-family indices.  -> dict(lines, passing, unique, ambiguous, uniq_reads and
        uniq_aln int64 [n_species], indptr int64 [ambiguous + 1], hit_species and hit_aln int32, side_cells, chunks, chunk_bytes,
        ms [8]; with dump: pid, score f64 and aln, qlen, species, marker int32 and passed uint8 per line).  A bad line raises
        MidasSnpsError with .bad = (reason, 1-based line), the earliest one of the file."""
        tx = np.frombuffer(text, np.uint8) if isinstance(text, (bytes, bytearray, memoryview)) else np.ascontiguousarray(text, dtype=np.uint8)
        names, off = _name_blob(gene_names)
        gs, gm = np.ascontiguousarray(gene_species, np.int32), np.ascontiguousarray(gene_marker, np.int32)
        cut = np.ascontiguousarray(marker_cutoff, np.float64)
        S = int(n_species)
        ur, ua = np.zeros(S, np.int64), np.zeros(S, np.int64)
        ip = np.array([chunk_bytes, hash_bits, 1 if dump else 0, 0], np.int64)
        res = C.c_void_p()
        stats, ms = self._device_call(self._lib.midas_species_classify, ptr(tx), tx.size, len(gene_names), ptr(names), ptr(off), ptr(gs),
                                      ptr(gm), S, cut.size, ptr(cut), float(aln_cov), ptr(ip), ptr(ur), ptr(ua), tail=(C.byref(res),), bad=2)
        try:
            n, n_amb, n_hits = int(stats[0]), int(stats[3]), int(stats[9])
            indptr, hs, ha = np.zeros(n_amb + 1, np.int64), np.zeros(n_hits, np.int32), np.zeros(n_hits, np.int32)
            self._check(self._lib.midas_species_result_columns(res, ptr(indptr), ptr(hs), ptr(ha)))
            out = dict(lines=n, passing=int(stats[1]), unique=int(stats[2]), ambiguous=n_amb, uniq_reads=ur, uniq_aln=ua, indptr=indptr,
                       hit_species=hs, hit_aln=ha, side_cells=int(stats[6]), chunks=int(stats[7]), chunk_bytes=int(stats[8]), ms=ms.tolist())
            if dump:
                cols = dict(pid=np.zeros(n, np.float64), score=np.zeros(n, np.float64), aln=np.zeros(n, np.int32), qlen=np.zeros(n, np.int32),
                            species=np.zeros(n, np.int32), marker=np.zeros(n, np.int32), passed=np.zeros(n, np.uint8))
                self._check(self._lib.midas_species_result_lines(res, *[ptr(cols[k]) for k in ('pid', 'score', 'aln', 'qlen', 'species', 'marker', 'passed')]))
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
        names, off = _name_blob(ids)
        if names.size == 0:
            names = np.zeros(1, np.uint8)      # (the entry point refuses a NULL blob even of no names: one byte to point at)
        ip = np.array([chunk_bytes, lds_bound, threads, 0], np.int64)
        res = C.c_void_p()
        stats, ms = self._device_call(self._lib.midas_species_merge, len(paths), C.cast(arr, C.c_void_p), len(ids), ptr(names), ptr(off),
                                      float(sample_depth), ptr(ip), tail=(C.byref(res),))
        return SpeciesMerge(self._lib, res, len(ids), len(paths), stats, ms)
