"""The commands over one species of `merge_midas.py snps`: snp_diversity.py, call_consensus.py, strain_tracking.py,
snp_pairs.py, snp_ld.py, snp_pnps.py and snp_trees.py's neighbour joining."""

from __future__ import annotations

import ctypes as C

import numpy as np

from .core import P, _GenesOwner, addr, columns, cstr, host_call, i32, i64, load_library, mt_states, ptr, register, vp, walk_stats

SITES_WEIGHT, SITES_ROUND, SITES_POOLED, SITES_PER_GENE, SITES_MASK_ONLY, SITES_SEQ, SITES_SUMS = 1, 2, 4, 8, 16, 32, 64
SITES_LD_SAME_GENE = 128     # MIDAS_SITES_LD_SAME_GENE
SITES_LD_MAX_BINS = 4096     # the most distance bins of midas_sites_ld
SITES_MAX_CLASSES = 4        # MIDAS_SITES_MAX_CLASSES
SITES_PAIR_TILE = 64         # MIDAS_SITES_PAIR_TILE: samples a side of the pair kernel's tile
ALLELE_LETTERS = 'ATCG'      # the order of the allele codes and of the count columns of strain_tracking.py id_markers

_text = [vp, vp, i64, vp, i64]                                          # handle, the two matrices' text and bytes
_scan = _text + [i64, vp, vp, vp, vp, i32] + [vp] * 15                  # midas_sites_scan's arguments, which two forms extend
_pairs = _text + [i64, vp, i32] + [vp] * 4                              # ... N, mask, S, columns, mean depth, fp, ip

# the analysis entry points (snp_diversity.py, call_consensus.py, strain_tracking.py, ...): listed by themselves (SITES_SYMBOLS)
register('sites', {
    'midas_sites_tables_open': (i32, [cstr, P(vp), cstr]),
    'midas_sites_tables_counts': (i32, [vp, vp]),
    'midas_sites_tables_columns': (i32, [vp, vp, vp]),
    'midas_sites_tables_close': (None, [vp]),
    'midas_sites_tables_positions': (i32, [vp, vp, vp, cstr]),
    'midas_sites_parse_cell': (i32, [i32, cstr, i64, vp]),
    'midas_sites_scan': (i32, _scan),
    'midas_sites_scan_resampled': (i32, _scan + [i64, i32, vp, i32, vp, vp, vp]),
    'midas_sites_scan_classes': (i32, _scan + [vp, i32]),
    'midas_sites_id_markers': (i32, _text + [i64, i64, vp, vp, i32] + [vp] * 6),
    'midas_sites_track_markers': (i32, _text + [i64, i64, vp, i32] + [vp] * 6),
    'midas_sites_consensus_pairs': (i32, _pairs + [vp] * 4),
    'midas_sites_pair_diversity': (i32, _pairs + [vp] * 9),
    'midas_sites_ld': (i32, _pairs + [vp, vp, i64, i64] + [vp] * 7),
    'midas_sites_write_markers': (i32, [cstr, vp, i64, vp, cstr]),
    'midas_sites_write_pairs': (i32, [cstr, vp, i32, vp, vp, cstr]),
})
# snp_trees.py (neighbour joining over the consensus distances): listed by itself (TREE_SYMBOLS)
register('tree', {
    'midas_nj_tree': (i32, [vp, i32] + [vp] * 7),
})


class SitesTables:
    """One species directory of `merge_midas.py snps` (midas_sites_tables_*): snps_summary.txt and snps_info.txt as columns,
    snps_freq.txt / snps_depth.txt mapped as text.  String columns are (.x_pool uint8, .x_off int64) pairs read through
    .strings(name); .freq_text / .depth_text are the matrices' rows after the header line.  Views owned by the handle."""

    STRING_COLUMNS = ('sample_id', 'site_id', 'ref_allele', 'major_allele', 'minor_allele', 'locus_type', 'site_type', 'gene_id',
                      'matrix_sample_id')

    def __init__(self, indir: str):
        lib = load_library()
        h = C.c_void_p()
        host_call(lib.midas_sites_tables_open, indir.encode(), C.byref(h), wide=True, what="midas_sites_tables_open")
        self._owner = _GenesOwner(lib, h, 'midas_sites_tables_close')
        self.dir = indir
        counts = (C.c_int64 * 8)()
        lib.midas_sites_tables_counts(h, counts)
        self.n_samples, self.n_sites, self.n_genes, self.n_columns = (int(counts[k]) for k in range(4))
        self.freq_columns = int(counts[6])
        ptrs, sizes = (C.c_void_p * 25)(), (C.c_int64 * 10)()
        lib.midas_sites_tables_columns(h, ptrs, sizes)
        col = columns(self._owner, ptrs)
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
            host_call(self._owner._lib.midas_sites_tables_positions, self._owner._h, ptrs, sizes, wide=True, what="midas_sites_tables_positions")
            col = columns(self._owner, ptrs)
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
        # (addr: no markers are an empty table to write the header over, not a missing argument)
        host_call(self._owner._lib.midas_sites_write_markers, path.encode(), self._owner._h, rows.shape[0], addr(rows),
                  wide=True, what="midas_sites_write_markers")

    def write_pairs(self, path: str, sample_rows, both):
        """The table of strain_tracking.py track_markers (midas_sites_write_pairs): both int64 [S, S] as Context.sites_track_markers
        returns it, sample_rows [S] = the samples' rows of snps_summary.txt."""
        rows = np.ascontiguousarray(sample_rows, dtype=np.int32)
        b = np.ascontiguousarray(both, dtype=np.int64)
        assert b.shape == (rows.shape[0], rows.shape[0])
        host_call(self._owner._lib.midas_sites_write_pairs, path.encode(), self._owner._h, rows.shape[0], addr(rows),
                  addr(b), wide=True, what="midas_sites_write_pairs")     # (as write_markers: no samples, the header alone)

    def first_bytes(self, name: str):
        """(first byte of every string, or 0 for an empty one; the lengths)."""
        pool, off = self._str[name]
        ln = off[1:] - off[:-1]
        if pool.shape[0] == 0:
            return np.zeros(ln.shape[0], np.uint8), ln
        first = pool[np.minimum(off[:-1], pool.shape[0] - 1)].copy()
        first[ln == 0] = 0
        return first, ln


def parse_cell(text: bytes, kind: str):
    """float() ('freq') or int() ('depth') of a matrix cell by the library's exact host parser; None when it is no number."""
    lib = load_library()
    if kind == 'freq':
        out = C.c_double(0)
        return float(out.value) if lib.midas_sites_parse_cell(0, text, len(text), C.byref(out)) == 0 else None
    out = C.c_int64(0)
    return int(out.value) if lib.midas_sites_parse_cell(1, text, len(text), C.byref(out)) == 0 else None


def _site_inputs(freq_text, depth_text, site_mask, sample_col, mean_depth, min_samples: int = 1):
    """The site commands' five inputs as the arrays the library takes -> ((freq text, depth text, mask, columns, mean depth),
    S, N).  Every command wants mean_depth [S]; all but sites_pair_diversity (min_samples 0) at least one sample."""
    ft = np.ascontiguousarray(freq_text, dtype=np.uint8)
    dt = np.ascontiguousarray(depth_text, dtype=np.uint8)
    mask = np.ascontiguousarray(site_mask, dtype=np.uint8)
    cols = np.ascontiguousarray(sample_col, dtype=np.int32)
    mean = np.ascontiguousarray(mean_depth, dtype=np.float64)
    S, N = int(cols.shape[0]), int(mask.shape[0])
    assert mean.shape[0] == S and S >= min_samples
    return (ft, dt, mask, cols, mean), S, N


def _pairs_head(arrays, S, N, fp, ip):
    """(freq text, bytes, depth text, bytes, N, mask, S, columns, mean depth, fp, ip): how consensus_pairs, pair_diversity and
    ld begin after the handle."""
    ft, dt, mask, cols, mean = arrays
    return (ptr(ft), ft.shape[0], ptr(dt), dt.shape[0], N, ptr(mask), S, ptr(cols), ptr(mean), ptr(fp), ptr(ip))


class _SitesCalls:
    """Context's site commands and the neighbour-joining tree."""

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
        (ft, dt, mask, cols, mean), S, N = _site_inputs(freq_text, depth_text, site_mask, sample_col, mean_depth)
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
        common = (ptr(ft), ft.shape[0], ptr(dt), dt.shape[0], N, ptr(mask), ptr(gene), ptr(mi), ptr(ma), S, ptr(cols), ptr(mean), ptr(fp),
                  ptr(ip), ptr(out.get('pi')), ptr(out.get('snps')), ptr(out.get('sites')), ptr(out.get('depth')), ptr(seq),
                  ptr(out.get('freq')), ptr(out.get('depthv')), ptr(out.get('keep')), ptr(out.get('pooled')))
        if rand_reads:
            state = np_state if np_state is not None else np.random.get_state()
            (_, _), (key, pos) = mt_states(np_state=state)
            key_out, pos_out, draw = np.zeros(624, np.uint32), C.c_int32(-1), np.zeros(8, np.float64)
            stats, ms = self._device_call(self._lib.midas_sites_scan_resampled, *common,
                                          tail=(int(rand_reads), int(bool(replace_reads)), ptr(key), pos, ptr(key_out), C.byref(pos_out), ptr(draw)))
        elif _classes is not None:
            cls = None if _classes[0] is None else np.ascontiguousarray(_classes[0], dtype=np.uint8)
            assert cls is None or cls.shape[0] == N
            stats, ms = self._device_call(self._lib.midas_sites_scan_classes, *common, tail=(ptr(cls), int(_classes[1])))
        else:
            stats, ms = self._device_call(self._lib.midas_sites_scan, *common)
        if rand_reads:
            out.update(np_state=(state[0], key_out, pos_out.value) + tuple(state[3:]), n_resampled=int(stats[11]), n_drew=int(stats[12]),
                       raw_made=int(draw[0]), accepted_used=int(draw[1]), raw_consumed=int(draw[2]), draw_ms=draw[3:].tolist())
        out.update(walk_stats(stats), n_kept=int(stats[1]), no_gene=int(stats[8]), ms=ms.tolist())
        n = out['n_sites']
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
        stats, ms = self._device_call(fn, ptr(ft), ft.shape[0], ptr(dt), dt.shape[0], int(n_parse), int(n_call),
                                      *[ptr(a) for a in site_arrays], cols.shape[0], ptr(cols), ptr(fp), ptr(ip), ptr(out))
        return dict(walk_stats(stats), ms=ms.tolist()), stats

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
        arrays, S, N = _site_inputs(freq_text, depth_text, site_mask, sample_col, mean_depth)
        fp = np.array([site_ratio, allele_support, site_prev, site_maf, 0.0], np.float64)
        ip = np.array([site_depth, max_sites, flags & SITES_MASK_ONLY, 0, group_rows, chunk_bytes, pair_blocks, 0], np.int64)
        both, diff = np.zeros((S, S), np.int64), np.zeros((S, S), np.int64)
        stats, ms = self._device_call(self._lib.midas_sites_consensus_pairs, *_pairs_head(arrays, S, N, fp, ip), ptr(both), ptr(diff),
                                      extra=('limit', 13, lambda v: v < S))
        return dict(walk_stats(stats), both=both, diff=diff, n_kept=int(stats[1]), word_pairs=int(stats[8]), pair_runs=int(stats[11]),
                    pair_steps=int(stats[12]), sample_limit=int(stats[13]), ms=ms.tolist())

    def sites_pair_diversity(self, freq_text, depth_text, site_mask, sample_col, mean_depth, site_depth: int, site_ratio: float,
                             allele_support: float, site_prev: float, site_maf: float, snp_maf: float = 0.01, max_sites: int = -1,
                             flags: int = 0, group_rows: int = 0, chunk_bytes: int = 0, pair_form: int = 0):
        """midas_sites_pair_diversity(): for every pair i < j of the samples what sites_scan gives under SITES_SUMS | SITES_POOLED
        with those two alone, and the sums over the sites both are kept at (sites_scan's arguments; of flags SITES_WEIGHT and
        SITES_ROUND count; max_sites is every pair's own).  -> dict(sites / snps / shared int64 [S, S], pi / w1 / w2 / x f64
        [S, S], filled above the diagonal; n_sites, n_masked, side_freq, side_depth, groups, pair_sites, pair_form (1 | 4 pairs a
        lane a side), tiles, sample_limit, ms [8]).  Errors as sites_consensus_pairs: .bad for a row, .limit for too many samples.
        pair_form 2 runs the 4 x 4 kernel (0, 1: one pair a lane, the faster one on an MI355X): the output does not depend on it."""
        arrays, S, N = _site_inputs(freq_text, depth_text, site_mask, sample_col, mean_depth, min_samples=0)
        fp = np.array([site_ratio, allele_support, site_prev, site_maf, snp_maf], np.float64)
        ip = np.array([site_depth, max_sites, flags & (SITES_WEIGHT | SITES_ROUND), 0, group_rows, chunk_bytes, pair_form, 0], np.int64)
        out = {k: np.zeros((S, S), np.int64) for k in ('sites', 'snps', 'shared')}
        out.update({k: np.zeros((S, S), np.float64) for k in ('pi', 'w1', 'w2', 'x')})
        stats, ms = self._device_call(self._lib.midas_sites_pair_diversity, *_pairs_head(arrays, S, N, fp, ip),
                                      *[ptr(out[k]) for k in ('sites', 'snps', 'shared', 'pi', 'w1', 'w2', 'x')],
                                      extra=('limit', 13, lambda v: v < S))
        out.update(walk_stats(stats), n_masked=int(stats[1]), pair_sites=int(stats[8]), pair_form=int(stats[11]), tiles=int(stats[12]),
                   sample_limit=int(stats[13]), ms=ms.tolist())
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
        arrays, S, n = _site_inputs(freq_text, depth_text, site_mask, sample_col, mean_depth)
        key = np.ascontiguousarray(site_key, dtype=np.int64)
        gene = None if site_gene is None else np.ascontiguousarray(site_gene, dtype=np.int32)
        assert key.shape[0] == n and (gene is None or gene.shape[0] == n)
        n_bins = -(-int(max_dist) // int(bin_width)) if max_dist >= 1 and bin_width >= 1 else 1
        fp = np.array([site_ratio, allele_support, site_prev, site_maf, 0.0], np.float64)
        ip = np.array([site_depth, max_sites, flags & (SITES_MASK_ONLY | SITES_LD_SAME_GENE), min_samples, group_rows, chunk_bytes, anchor_chunk, 0],
                      np.int64)
        out = {k: np.zeros(n_bins, np.int64) for k in ('window', 'pairs')}
        out.update({k: np.zeros(n_bins, np.float64) for k in ('sum_r2', 'sum_d2', 'sum_het')})
        stats, ms = self._device_call(self._lib.midas_sites_ld, *_pairs_head(arrays, S, n, fp, ip), ptr(key), ptr(gene), int(max_dist),
                                      int(bin_width), *[ptr(out[k]) for k in ('window', 'pairs', 'sum_r2', 'sum_d2', 'sum_het')],
                                      extra=('limit', 13, lambda v: v > 0))
        out.update(walk_stats(stats), n_kept=int(stats[1]), pairs_visited=int(stats[8]), anchor_chunks=int(stats[11]),
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
        stats, ms = self._device_call(self._lib.midas_nj_tree, n, ptr(d), ptr(join), ptr(length), ptr(last), ptr(last_len), bad=0,
                                      extra=('limit', 0, lambda v: 0 < v < n))
        return dict(join=join, len=length, last=last, last_len=last_len, sample_limit=int(stats[0]), ms=ms.tolist())
