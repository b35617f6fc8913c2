"""run_midas.py genes (the per-gene counts) and the commands over merged gene matrices: compare_genes.py, gene_linkage.py,
gene_assoc.py, gene_curves.py."""

from __future__ import annotations

import ctypes as C

import numpy as np

from .core import (ERR_INVALID_ARG, MidasSnpsError, P, _GenesOwner, addr, columns, cstr, f64, host_call, i32, i64, load_library, ptr,
                   register, text_buffer, vp, walk_stats)
from .pileup import Thresholds
from .reads import ResidentReads, _Reads

GENES_BAM_PHASES = ('upload', 'inflate + crc', 'walk + stitch + offsets', 'facts kernel', 'filter + sort + sums', 'download')
GENES_BAM_STATS = ('records', 'dropped', 'blocks', 'inflated_bytes', 'chunks', 'chunks_again')
GENES_DTYPES = {'presabs': 0, 'copynum': 1}                            # MIDAS_GENES_PRESABS / _COPYNUM
GENES_DISTANCES = {'jaccard': 0, 'euclidean': 1, 'manhattan': 2}       # MIDAS_GENES_JACCARD / _EUCLIDEAN / _MANHATTAN

_count = [vp, P(Thresholds), P(_Reads), vp, i64, vp, vp, vp, vp, P(C.c_float)]      # of genes_count and genes_count_device

register('exported', {
    'midas_genes_count': (i32, _count),
    'midas_genes_terms': (i32, [vp, P(Thresholds), P(_Reads), vp, i64, vp, vp, P(C.c_float)]),
    'midas_genes_count_device': (i32, _count),
    'midas_genes_count_timing': (i32, [vp, vp]),
    'midas_genes_count_bam': (i32, [vp, vp, P(Thresholds), i64, vp, vp, vp, vp, vp, vp, cstr]),
    'midas_genes_sum': (i32, [vp, i64, vp, vp, i64, vp, vp, vp, P(C.c_float)]),
    'midas_genes_matrix_open': (i32, [cstr, P(vp), cstr]),
    'midas_genes_matrix_counts': (i32, [vp, vp]),
    'midas_genes_matrix_columns': (i32, [vp, vp, P(i64)]),
    'midas_genes_matrix_close': (None, [vp]),
    'midas_genes_compare_parse_cell': (i32, [cstr, i64, P(f64), P(i32)]),
    'midas_genes_compare': (i32, [vp, vp, i64, i64, i32, i32, i32, i32, f64] + [vp] * 9),
    'midas_genes_compare_write_pairs': (i32, [cstr, vp, i32, i32, i32, i64, vp, vp, vp, vp, cstr]),
    'midas_genes_linkage': (i32, [vp, vp, i64, i64, i32, i32, f64, vp, vp, i64] + [vp] * 8),
    'midas_genes_linkage_write_pairs': (i32, [cstr, vp, i64, vp, vp, i64, vp, vp, vp, cstr]),
    'midas_genes_linkage_write_groups': (i32, [cstr, vp, i64, vp, vp, vp, i64, P(i64), cstr]),
    'midas_genes_assoc': (i32, [vp, vp, i64, i64, i32, i32, vp, vp, vp, i64, f64] + [vp] * 10),
    'midas_genes_assoc_write': (i32, [cstr, vp, i64] + [vp] * 6 + [i64, vp, vp, vp, cstr]),
    'midas_genes_curves': (i32, [vp, vp, i64, i64, i32, i32, vp, i64, i32, vp, f64] + [vp] * 6),
    'midas_genes_curves_write': (i32, [cstr, vp, i32, i64, i32, vp, vp, vp, vp, i64, vp, vp, cstr]),
})


class GenesMatrix:
    """One genes_<kind>.txt of `merge_midas.py genes` (midas_genes_matrix_*): mapped, not parsed.  .first_field and .sample_ids
    from the header line, .n_rows data rows, .text the rows after the header (uint8 view owned by the handle)."""

    def __init__(self, path: str):
        lib = load_library()
        h = C.c_void_p()
        host_call(lib.midas_genes_matrix_open, path.encode(), C.byref(h), wide=True, what="midas_genes_matrix_open")
        self._owner = _GenesOwner(lib, h, 'midas_genes_matrix_close')
        self.path = path
        counts = (C.c_int64 * 4)()
        lib.midas_genes_matrix_counts(h, counts)
        self.n_columns, self.n_rows = int(counts[0]), int(counts[1])
        ptrs, nfirst = (C.c_void_p * 4)(), C.c_int64(0)
        lib.midas_genes_matrix_columns(h, ptrs, C.byref(nfirst))
        col = columns(self._owner, ptrs)
        pool = col(0, int(counts[3]), np.uint8).tobytes()
        off = col(1, self.n_columns + 1, np.int64)
        self.sample_ids = [pool[int(off[k]):int(off[k + 1])].decode('utf-8', errors='surrogateescape') for k in range(self.n_columns)]
        self.text = col(2, int(counts[2]), np.uint8)
        self.first_field = C.string_at(ptrs[3], nfirst.value).decode('utf-8', errors='surrogateescape') if nfirst.value else ''

    def _write(self, fn_name: str, path: str, *args):
        host_call(getattr(self._owner._lib, fn_name), path.encode(), self._owner._h, *args, wide=True, what=fn_name)

    def write_pairs(self, path: str, res: dict):
        """The table of compare_genes.py (midas_genes_compare_write_pairs) from what Context.genes_compare returned."""
        arr = lambda k, dt: None if res.get(k) is None else np.ascontiguousarray(res[k], dtype=dt)
        count, both, either, dist = arr('count', np.int64), arr('both', np.float64), arr('either', np.float64), arr('dist', np.float64)
        self._write('midas_genes_compare_write_pairs', path, int(res['n_samples']), GENES_DTYPES[res['dtype']],
                    GENES_DISTANCES[res['distance']], int(res['n_rows']), ptr(count), ptr(both), ptr(either), ptr(dist))

    def write_linkage(self, path: str, res: dict):
        """The pair table of gene_linkage.py (midas_genes_linkage_write_pairs) from what Context.genes_linkage returned."""
        arr = lambda k: np.ascontiguousarray(res[k], dtype=np.int32)
        count, row, a, b, both = arr('count'), arr('row_of_slot'), arr('pair_a'), arr('pair_b'), arr('pair_both')
        self._write('midas_genes_linkage_write_pairs', path, count.shape[0], ptr(count), ptr(row), a.shape[0], ptr(a), ptr(b), ptr(both))

    def write_groups(self, path: str, res: dict, min_group: int = 2) -> int:
        """The group table of gene_linkage.py (midas_genes_linkage_write_groups) -> the groups written."""
        arr = lambda k: np.ascontiguousarray(res[k], dtype=np.int32)
        count, row, label = arr('count'), arr('row_of_slot'), arr('label')
        n = C.c_int64(0)
        self._write('midas_genes_linkage_write_groups', path, count.shape[0], ptr(count), ptr(row), ptr(label), int(min_group), C.byref(n))
        return int(n.value)

    def write_assoc(self, path: str, res: dict, table: dict):
        """The table of gene_assoc.py (midas_genes_assoc_write) from what Context.genes_assoc returned and the host's columns:
        table = dict(effect, p_value, q_value f64 [K] and, with permutations, p_perm, q_perm)."""
        i32a = lambda k: np.ascontiguousarray(res[k], dtype=np.int32)
        f64a = lambda k: None if table.get(k) is None else np.ascontiguousarray(table[k], dtype=np.float64)
        row, count, case = i32a('row_of_slot'), i32a('count'), i32a('count_case')
        n_perms = int(res['n_perms'])
        exceed = np.ascontiguousarray(res['exceed'], dtype=np.uint32) if n_perms else None
        cols = [f64a(k) for k in ('effect', 'p_value', 'q_value', 'p_perm', 'q_perm')]
        self._write('midas_genes_assoc_write', path, row.shape[0], ptr(row), ptr(count), ptr(case), ptr(cols[0]), ptr(cols[1]),
                    ptr(cols[2]), n_perms, ptr(exceed), ptr(cols[3]), ptr(cols[4]))

    def _write_curves(self, path: str, which: int, res: dict, orders=None, table=None):
        """Either table of gene_curves.py (midas_genes_curves_write) from what genes_curves returned."""
        i64a = lambda a: np.ascontiguousarray(a, dtype=np.int64)
        pan, core, single = i64a(res['pan']), i64a(res['core']), i64a(res['single'])
        R, N = pan.shape
        od = None if orders is None else np.ascontiguousarray(orders, dtype=np.int32)
        if pan.shape != core.shape or pan.shape != single.shape or (od is not None and od.shape != pan.shape):
            raise MidasSnpsError(ERR_INVALID_ARG, "pan, core, single and orders must be [orders, samples in use] alike")
        n_perms = R - 1 if table else 0
        means = minmax = None
        if n_perms:
            means = np.ascontiguousarray([table[k] for k in ('pan_mean', 'core_mean', 'single_mean', 'new_mean')], dtype=np.float64)
            minmax = np.ascontiguousarray([table[k] for k in ('pan_min', 'pan_max', 'core_min', 'core_max', 'single_min', 'single_max')],
                                          dtype=np.int64)
            if means.shape != (4, N) or minmax.shape != (6, N):
                raise MidasSnpsError(ERR_INVALID_ARG, "every statistic column must hold one entry a sample in use")
        self._write('midas_genes_curves_write', path, which, R, N, ptr(pan), ptr(core), ptr(single), ptr(od), n_perms, ptr(means), ptr(minmax))

    def write_curves(self, path: str, res: dict, table: dict):
        """The curve table of gene_curves.py from what genes_curves returned and the host's columns: table = dict(pan_mean,
        core_mean, single_mean, new_mean f64 [N]; pan_min, pan_max, core_min, core_max, single_min, single_max int64 [N]), or an
        empty dict when there is no random order."""
        self._write_curves(path, 0, res, table=table)

    def write_curve_orders(self, path: str, res: dict, orders):
        """The table of every order of gene_curves.py: one row an (order, k) with the id of the sample added at that step."""
        self._write_curves(path, 1, res, orders=orders)


def pandas_cell(text: bytes):
    """A matrix cell as pandas' C reader converts it, by the library's host build of the device converter
    (midas_genes_compare_parse_cell) -> (value, plain_int), or None when it is no finite decimal literal."""
    lib = load_library()
    out, plain = C.c_double(0), C.c_int32(0)
    if lib.midas_genes_compare_parse_cell(text, len(text), C.byref(out), C.byref(plain)) != 0:
        return None
    return float(out.value), bool(plain.value)


def _matrix_text(text, n_rows, n_samples, n_columns):
    """The gene commands' (text, n_rows, n_samples, n_columns) -> the text as a uint8 array, N, S and the first arguments of
    the call after the handle."""
    tx = np.ascontiguousarray(text, dtype=np.uint8)
    N, S = int(n_rows), int(n_samples)
    return tx, N, S, (ptr(tx), tx.shape[0], N, S, int(n_columns))


def genes_curves(ctx, text, n_rows: int, n_samples: int, n_columns: int, orders, need, cutoff: float = 0.35, form: int = 1,
                 group_rows: int = 0, chunk_bytes: int = 0, out=None):
    """midas_genes_curves() on the context ctx: gene_curves.py over the text rows of genes_copynum.txt, the first n_samples of
    n_columns sample columns, rows [0, n_rows).  orders: int32 [R, N], row 0 the columns in use, every other row a permutation
    of them; need: int32 [N + 1], 1 <= need[k] <= k.  -> dict(n_rows read, n_samples, n_used N, n_orders R, pan, core, single
    int64 [R, N], groups, group_rows, chunk_bytes, form, planes, words, ms [8]).  A broken rule of orders or need raises
    MidasSnpsError (ERR_INVALID_ARG) whose message names the row, a malformed row of the matrix raises it with .bad as
    Context.genes_compare.  out (tests): three int64 [R, N] arrays to receive pan, core and single."""
    tx, n, S, head = _matrix_text(text, n_rows, n_samples, n_columns)
    od = np.ascontiguousarray(orders, dtype=np.int32)
    nd = np.ascontiguousarray(need, dtype=np.int32)
    if od.ndim != 2 or od.shape[0] < 1 or od.shape[1] < 1:
        raise MidasSnpsError(ERR_INVALID_ARG, "orders must be [orders, samples in use], one row at least")
    R, N = od.shape
    if nd.shape != (N + 1,):
        raise MidasSnpsError(ERR_INVALID_ARG, "need must hold one entry more than a row of orders")
    pan, core, single = out if out is not None else (np.zeros((R, N), np.int64), np.zeros((R, N), np.int64), np.zeros((R, N), np.int64))
    for a in (pan, core, single):
        if a.dtype != np.int64 or a.shape != (R, N) or not a.flags.c_contiguous:
            raise MidasSnpsError(ERR_INVALID_ARG, "out must be three contiguous int64 arrays shaped as orders")
    ip = np.array([group_rows, chunk_bytes, form, 0, 0, 0, 0, 0], np.int64)
    stats, ms = ctx._device_call(ctx._lib.midas_genes_curves, *head, ptr(od), R, N, ptr(nd), float(cutoff), ptr(ip), ptr(pan), ptr(core),
                                 ptr(single))
    return dict(walk_stats(stats, 'n_rows', side=False), n_samples=S, n_used=N, n_orders=R, pan=pan, core=core, single=single,
                form=int(stats[13]), planes=int(stats[14]), words=int(stats[8]), ms=ms.tolist())


class _GenesCalls:
    """Context's gene commands."""

    def _genes_counts(self, fn, thr, reads, ref_id, gene_length):
        """genes_count and genes_count_device: one signature, host or device payload."""
        rid = np.ascontiguousarray(ref_id, dtype=np.int32)
        gl = np.ascontiguousarray(gene_length, dtype=np.int64)
        n = gl.shape[0]
        aligned, mapped, depth = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.float64)
        ms = C.c_float(0)
        r = reads._c()
        # (addr: no reads, or no genes, are empty arrays beside a count of 0)
        self._check(fn(self._h, C.byref(thr), C.byref(r), addr(rid), n, addr(gl), addr(aligned), addr(mapped), addr(depth), C.byref(ms)))
        return aligned, mapped, depth, float(ms.value)

    def genes_count(self, thr: Thresholds, reads: "ReadsSoA", ref_id, gene_length):
        """midas_genes_count(): per gene (aligned_reads i64, mapped_reads i64, depth f64, kernel_ms)."""
        return self._genes_counts(self._lib.midas_genes_count, thr, reads, ref_id, gene_length)

    def genes_count_device(self, thr: Thresholds, reads: "ReadsSoA", ref_id, gene_length):
        """midas_genes_count_device(): genes_count over a ReadsSoA whose QUAL / CIGAR lie on this context's device (read_sam(...,
        order='file'), read_bam(..., payload_on_device=True), BamSlice.load_ranges(ctx=...)); the per-read facts are made there."""
        if isinstance(reads, ResidentReads):
            reads = reads.to_columns(self)
        if reads.device is None:
            raise MidasSnpsError(ERR_INVALID_ARG, "genes_count_device takes reads whose payload is on the device (genes_count takes host columns)")
        return self._genes_counts(self._lib.midas_genes_count_device, thr, reads, ref_id, gene_length)

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
        # (the message goes to the context as well, where _check reads it; addr: a header of no references)
        st = self._lib.midas_genes_count_bam(self._h, handle._h, C.byref(thr), n, addr(gl), addr(aligned), addr(mapped), addr(depth),
                                             ptr(stats), ptr(ms), text_buffer())
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
        st = self._lib.midas_genes_terms(self._h, C.byref(thr), C.byref(r), addr(rid), gl.shape[0], addr(gl), addr(term), C.byref(ms))
        self._check(st)
        return term

    def genes_sum(self, gene, term, n_genes):
        """midas_genes_sum(): (gene, term) pairs in BAM order -> per gene (aligned_reads i64, mapped_reads i64, depth f64)."""
        g = np.ascontiguousarray(gene, dtype=np.int32)
        t = np.ascontiguousarray(term, dtype=np.float64)
        n = int(n_genes)
        aligned, mapped, depth = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.float64)
        ms = C.c_float(0)
        st = self._lib.midas_genes_sum(self._h, g.shape[0], addr(g), addr(t), n, addr(aligned), addr(mapped), addr(depth), C.byref(ms))
        self._check(st)
        return aligned, mapped, depth

    def genes_compare(self, text, n_rows: int, n_samples: int, n_columns: int, dtype: str = 'presabs', distance: str = 'jaccard',
                      cutoff: float = 0.35, group_rows: int = 0, chunk_bytes: int = 0, pair_blocks: int = 0, dump: bool = False):
        """midas_genes_compare(): compare_genes.py over the text rows of genes_copynum.txt, the first n_samples of n_columns sample
        columns, rows [0, n_rows).  -> dict(dtype, distance, n_samples, n_rows read, col_float uint8 [S], groups, steps, tiles,
        group_rows, chunk_bytes, ms [8]; presabs: count int64 [S, S]; copynum: both, either and (euclidean / manhattan) dist f64
        [S, S], all filled for i <= j; with dump: cells f64 [S, n_rows]).  A malformed row raises MidasSnpsError with
        .bad = (1 width | 2 cell, data row, sample column or -1)."""
        tx, N, S, head = _matrix_text(text, n_rows, n_samples, n_columns)
        copynum = dtype == 'copynum'
        kd = GENES_DISTANCES[distance]
        count = None if copynum else np.zeros((S, S), np.int64)
        both = np.zeros((S, S), np.float64) if copynum else None
        either = np.zeros((S, S), np.float64) if copynum else None
        dist = np.zeros((S, S), np.float64) if copynum and kd else None
        col_float = np.zeros(S, np.uint8)
        cells = np.zeros((S, max(N, 1)), np.float64) if dump else None
        ip = np.array([group_rows, chunk_bytes, pair_blocks, 0], np.int64)
        stats, ms = self._device_call(self._lib.midas_genes_compare, *head, GENES_DTYPES[dtype], kd, float(cutoff), ptr(ip),
                                      ptr(count), ptr(both), ptr(either), ptr(dist), ptr(col_float), ptr(cells))
        out = dict(walk_stats(stats, 'n_rows', side=False), dtype=dtype, distance=distance, n_samples=S, col_float=col_float,
                   steps=int(stats[8]), tiles=int(stats[11]), ms=ms.tolist(), count=count, both=both, either=either, dist=dist)
        if dump:
            out['cells'] = cells[:, :out['n_rows']]
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
        tx, N, S, head = _matrix_text(text, n_rows, n_samples, n_columns)
        cap = int(max_pairs)
        nd = np.ascontiguousarray(need, dtype=np.int32)
        if nd.shape != (S + 1,):
            raise MidasSnpsError(ERR_INVALID_ARG, "need must hold n_samples + 1 entries")
        count, row, label = np.zeros(N, np.int32), np.zeros(N, np.int32), np.zeros(N, np.int32)
        pa, pb, pc = pair_out if pair_out is not None else (np.empty(cap, np.int32), np.empty(cap, np.int32), np.empty(cap, np.int32))
        ip = np.array([group_rows, chunk_bytes, min_present, min_absent, pair_form, 0, 0, 0], np.int64)
        stats, ms = self._device_call(self._lib.midas_genes_linkage, *head, float(cutoff), ptr(ip), ptr(nd), cap, ptr(count),
                                      ptr(row), ptr(label), ptr(pa), ptr(pb), ptr(pc), extra=('linked', 11, lambda v: v > cap))
        K, n = int(stats[1]), int(stats[11])
        return dict(walk_stats(stats, 'n_rows', side=False), n_samples=S, n_kept=K, count=count[:K], row_of_slot=row[:K], label=label[:K],
                    pair_a=pa[:n].copy(), pair_b=pb[:n].copy(), pair_both=pc[:n].copy(), visited=int(stats[8]), linked=n,
                    label_rounds=int(stats[12]), form=int(stats[13]), strips=int(stats[14]), ms=ms.tolist())

    def genes_assoc(self, text, n_rows: int, n_samples: int, n_columns: int, use, case, planes, cutoff: float = 0.35,
                    dtype: str = 'presabs', min_present: int = 1, min_absent: int = 0, group_rows: int = 0, chunk_bytes: int = 0,
                    form: int = 1, products: bool = False):
        """midas_genes_assoc(): gene_assoc.py over the text rows of genes_copynum.txt, the first n_samples of n_columns sample
        columns, rows [0, n_rows).  use, case: uint64 [ceil(n_samples / 64)], bit s: column s takes part / is a case; planes:
        uint64 [P, ceil(n_samples / 64)], the relabellings (P may be 0).  -> dict(n_rows read, n_samples, n_used N, n_case n1,
        n_perms P, dtype, n_kept K, row_of_slot, count, count_case int32 [K], w, ties int64 [K], exceed uint32 [K], groups,
        group_rows, chunk_bytes, form, in_lds, ms [8]; with products (tests): products int32 [K, P]).  A malformed row raises
        MidasSnpsError with .bad as genes_compare."""
        tx, N, S, head = _matrix_text(text, n_rows, n_samples, n_columns)
        W = (S + 63) // 64
        us, cs = np.ascontiguousarray(use, dtype=np.uint64), np.ascontiguousarray(case, dtype=np.uint64)
        pl = np.ascontiguousarray(planes, dtype=np.uint64).reshape(-1, W)
        if us.shape != (W,) or cs.shape != (W,):
            raise MidasSnpsError(ERR_INVALID_ARG, "use and case must hold ceil(n_samples / 64) words")
        n_perms = pl.shape[0]
        row, count, ccase = np.zeros(N, np.int32), np.zeros(N, np.int32), np.zeros(N, np.int32)
        w, ties, exceed = np.zeros(N, np.int64), np.zeros(N, np.int64), np.zeros(N, np.uint32)
        prod = np.zeros(min(N * n_perms, 1 << 24), np.int32) if products else None
        ip = np.array([group_rows, chunk_bytes, min_present, min_absent, GENES_DTYPES[dtype], form, 0, 0], np.int64)
        # (addr: with n_samples 0 use and case are empty, and the entry point still wants the two arguments given)
        stats, ms = self._device_call(self._lib.midas_genes_assoc, *head, addr(us), addr(cs), ptr(pl), n_perms, float(cutoff), ptr(ip),
                                      ptr(row), ptr(count), ptr(ccase), ptr(w), ptr(ties), ptr(exceed), ptr(prod))
        K = int(stats[1])
        out = dict(walk_stats(stats, 'n_rows', side=False), n_samples=S, n_used=int(stats[11]), n_case=int(stats[12]), n_perms=n_perms,
                   dtype=dtype, n_kept=K, row_of_slot=row[:K], count=count[:K], count_case=ccase[:K], w=w[:K], ties=ties[:K],
                   exceed=exceed[:K], form=int(stats[13]), in_lds=int(stats[8]), ms=ms.tolist())
        if products:
            out['products'] = prod[:K * n_perms].reshape(K, n_perms).copy()
        return out
