"""merge_midas.py snps and genes: the samples' tables on the device, the site merge and its writers, the gene merge."""

from __future__ import annotations

import ctypes as C

import numpy as np

from .core import ERR_UNSUPPORTED, MidasSnpsError, P, _GenesOwner, addr, columns, cstr, f64, host_call, i32, i64, load_library, ptr, \
    register, vp
from .pileup import _TableSet

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

TABLES_READ_PHASES = ('upload', 'inflate + crc', 'index', 'parse')
TABLES_READ_STATS = ('tables', 'members', 'groups', 'compressed_bytes', 'inflated_bytes', 'rows', 'groups_decoded_twice')
GENES_MATRIX_KINDS = {'presabs': 0, 'copynum': 1, 'depth': 1, 'reads': 2}


class _Genes(C.Structure):
    _fields_ = [("n_genes", C.c_int64), ("scaffold_id", C.c_void_p), ("start", C.c_void_p), ("end", C.c_void_p),
                ("strand", C.c_char_p), ("gene_type", C.c_void_p), ("gene_id", C.c_void_p), ("seq", C.c_void_p)]


_tables_tail = [cstr, cstr, cstr, i64, vp, vp, vp, P(i64), P(C.c_float), P(C.c_float)]     # of the two merge_sites_tables forms

register('exported', {
    'midas_merge_write_info': (i32, [cstr, cstr, i64, vp, vp, vp, vp, vp, vp, vp, i32, i64, cstr]),
    'midas_merge_write_matrix': (i32, [cstr, cstr, i64, vp, i32, i64, vp, vp, i32, i64, cstr]),
    'midas_merge_write_matrix_device': (i32, [vp, cstr, cstr, i64, vp, i32, i64, vp, vp, i64, P(C.c_float)]),
    'midas_merge_sites': (i32, [vp, P(MergeParams), i32, i64, P(vp), vp] + [vp] * 5 + [P(C.c_float)]),
    'midas_merge_sites_tables': (i32, [vp, P(MergeParams), i32, i64, P(vp), vp] + _tables_tail),
    'midas_merge_sites_resident': (i32, [vp, P(MergeParams), vp, i64, vp] + [vp] * 5 + [P(C.c_float)]),
    'midas_merge_sites_tables_resident': (i32, [vp, P(MergeParams), vp, i64, vp] + _tables_tail),
    'midas_merge_tables_create': (i32, [vp, i32, i64, P(vp)]),
    'midas_merge_tables_free': (None, [vp]),
    'midas_merge_tables_shape': (i32, [vp, P(i32), P(i64)]),
    'midas_merge_tables_set_host': (i32, [vp, vp, i32, i64, vp]),
    'midas_merge_tables_fetch': (i32, [vp, vp, i32, i64, vp]),
    'midas_snps_tableset_read_counts_device': (i32, [vp, vp, i64, i64, i32, vp, vp, vp, cstr]),
    'midas_snps_parse_rows_device': (i32, [vp, vp, i64, i32, vp, i64, P(i64), P(i64)]),
    'midas_genes_merge_map_open': (i32, [cstr, cstr, P(vp), cstr]),
    'midas_genes_merge_map_n_clusters': (i64, [vp]),
    'midas_genes_merge_map_n_genes': (i64, [vp]),
    'midas_genes_merge_map_columns': (i32, [vp, vp, vp]),
    'midas_genes_merge_map_close': (None, [vp]),
    'midas_genes_merge_tables_open': (i32, [i32, vp, i32, P(vp), cstr]),
    'midas_genes_merge_tables_rows': (i64, [vp, i32]),
    'midas_genes_merge_tables_resolve': (i32, [vp, vp, i32, i32, cstr]),
    'midas_genes_merge_tables_columns': (i32, [vp, i32, vp, P(i64), P(i32)]),
    'midas_genes_merge_tables_close': (None, [vp]),
    'midas_genes_merge': (i32, [vp, i32, vp, vp, vp, vp, vp, i64, f64, i32, i64, P(i64)] + [vp] * 5 + [P(C.c_float)]),
    'midas_genes_merge_write_matrix': (i32, [cstr, cstr, i32, i64, vp, vp, vp, i32, vp, vp, i32, cstr]),
    'midas_genes_merge_format_f64': (i32, [i64, vp, vp, i64, P(i64)]),
})


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
    gs = _Genes(n, C.cast(sid, C.c_void_p), addr(start), addr(end), strand,
                C.cast(gty, C.c_void_p), C.cast(gid, C.c_void_p), C.cast(seq, C.c_void_p))
    # (addr: a species of no kept sites, or of no genes, still gets its file from these arrays)
    host_call(lib.midas_merge_write_info, path.encode(), header_line.encode(), keep.shape[0], addr(keep), addr(kb), addr(key_off),
              addr(calls), addr(cs), addr(pooled), C.byref(gs), int(threads), int(site_id_base))


def _matrix_inputs(keep, depth, minor_count):
    """keep int64, depth and minor_count (or None) uint32 [S, n] of the two matrix writers, and S, n."""
    keep = np.ascontiguousarray(keep, dtype=np.int64)
    depth = np.ascontiguousarray(depth, dtype=np.uint32)
    mc = None
    if minor_count is not None:
        mc = np.ascontiguousarray(minor_count, dtype=np.uint32)
        assert mc.shape == depth.shape
    return (keep, depth, mc) + depth.shape


def write_merge_matrix(path: str, header_line: str, keep: np.ndarray, depth: np.ndarray, minor_count=None, threads: int = 0,
                       site_id_base: int = 0):
    """snps_depth.txt (minor_count None) / snps_freq.txt of merge_midas.py snps for the kept sites (midas_merge_write_matrix).
    depth, minor_count: [n_samples, n_sites] uint32 as returned by Context.merge_sites."""
    lib = load_library()
    keep, depth, mc, S, n = _matrix_inputs(keep, depth, minor_count)
    # (addr: a NULL minor_count says "the depth file"; no kept sites still write the header)
    host_call(lib.midas_merge_write_matrix, path.encode(), header_line.encode(), keep.shape[0], addr(keep), S, n, addr(depth), addr(mc),
              int(threads), int(site_id_base))


def write_merge_matrix_device(ctx, path: str, header_line: str, keep: np.ndarray, depth: np.ndarray, minor_count=None,
                              site_id_base: int = 0) -> float:
    """write_merge_matrix with the rows formatted on ctx's device (midas_merge_write_matrix_device): the same file, byte for
    byte.  Stricter than the host writer where the device needs it (MidasSnpsError): every keep[r] in [0, n_sites),
    site_id_base >= 0, no minor count above its non-zero depth, kept rows ascending unless the arrays fit one upload chunk
    (none of which merge_sites' outputs can violate).  -> device time of the formatter, ms."""
    keep, depth, mc, S, n = _matrix_inputs(keep, depth, minor_count)
    ms = C.c_float(0)
    st = ctx._lib.midas_merge_write_matrix_device(ctx._h, path.encode(), header_line.encode(), keep.shape[0], addr(keep), S, n,
                                                  addr(depth), addr(mc), int(site_id_base), C.byref(ms))
    ctx._check(st)
    return float(ms.value)


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
        self._ctx._check(self._lib.midas_merge_tables_set_host(self._ctx._h, self._h, int(sample), a.shape[0], addr(a)))

    def fetch(self, sample: int, n_rows: int = None):
        n = self.n_sites if n_rows is None else int(n_rows)
        out = np.empty((n, 4), np.uint32)
        self._ctx._check(self._lib.midas_merge_tables_fetch(self._ctx._h, self._h, int(sample), n, addr(out)))
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


class GeneClusterMap:
    """read_cluster_map (midas/merge/genes.py:91-98) read natively (midas_genes_merge_map_*): gene_info.txt[.gz] ->
    centroid_99 -> `cluster_column`.  .cluster_ids / .cluster_off: the distinct clusters in sorted byte order (index = output
    row order); .gene_ids / .gene_off / .gene_cluster: the distinct centroid_99 ids in first-appearance order and their
    clusters.  Read-only views owned by the handle."""

    def __init__(self, path: str, cluster_column: str):
        lib = load_library()
        h = C.c_void_p()
        host_call(lib.midas_genes_merge_map_open, path.encode(), cluster_column.encode(), C.byref(h), wide=True, what="midas_genes_merge_map_open")
        self._owner = _GenesOwner(lib, h, 'midas_genes_merge_map_close')
        self.path = path
        self.n_clusters = int(lib.midas_genes_merge_map_n_clusters(h))
        self.n_genes = int(lib.midas_genes_merge_map_n_genes(h))
        ptrs, sizes = (C.c_void_p * 5)(), (C.c_int64 * 2)()
        lib.midas_genes_merge_map_columns(h, ptrs, sizes)
        col = columns(self._owner, ptrs)
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
        host_call(lib.midas_genes_merge_tables_open, n, c_paths, int(threads), C.byref(h), wide=True, what="midas_genes_merge_tables_open")
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
            col = columns(self._owner, ptrs)
            self.ids.append(col(0, int(nb.value), np.uint8))
            self.id_off.append(col(1, n + 1, np.int64))
            self.copy.append(col(2, n, np.float64))
            self.depth.append(col(3, n, np.float64))
            self.reads.append(col(4, n, np.int64))
            self.cluster.append(col(5, n, np.uint32) if self.resolved else None)
            self.same_as.append(int(same.value))

    def resolve(self, cmap: "GeneClusterMap", reuse: bool = True, threads: int = 0):
        host_call(self._lib.midas_genes_merge_tables_resolve, self._owner._h, cmap.handle, 1 if reuse else 0, int(threads), wide=True,
                  what="midas_genes_merge_tables_resolve")
        self.resolved = True
        self._columns()     # (a sample that shares an earlier one's vector views the same memory: one class on the device)


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
    host_call(lib.midas_genes_merge_write_matrix, path.encode(), header_line.encode(), k, R, ptr(rc), ptr(cmap.cluster_ids),
              ptr(cmap.cluster_off), S, ptr(vals), ptr(st_), int(threads), wide=True)


def format_repr_f64(values) -> list:
    """Python's repr() of every double, by the matrix writer's formatter (midas_genes_merge_format_f64)."""
    lib = load_library()
    v = np.ascontiguousarray(values, dtype=np.float64)
    out = np.empty(33 * v.shape[0] + 1, np.uint8)
    n = C.c_int64(0)
    st = lib.midas_genes_merge_format_f64(v.shape[0], addr(v), ptr(out), out.shape[0], C.byref(n))      # (addr: no values format to nothing)
    if st != 0:
        raise MidasSnpsError(st, "midas_genes_merge_format_f64 failed")
    return out[:n.value].tobytes().decode().split('\n')[:-1]


class _MergeCalls:
    """Context's merge commands: the device readers of the samples' tables, merge_sites and genes_merge."""

    def parse_rows(self, text: bytes, skip_header: bool = True, cap_rows: int = None):
        """The device's row parser on the text of one table (midas_snps_parse_rows_device) -> (counts[n,4] u32 of the first cap_rows
        rows, rows found, first malformed row among them or -1)."""
        buf = np.frombuffer(text, np.uint8)
        cap = int(cap_rows) if cap_rows is not None else text.count(b"\n") + 1
        out = np.zeros((cap, 4), np.uint32)
        rows, bad = C.c_int64(0), C.c_int64(-1)
        # (addr: cap_rows 0 hands the parser an empty table to fill, not "no table")
        self._check(self._lib.midas_snps_parse_rows_device(self._h, ptr(buf), buf.size, 1 if skip_header else 0, addr(out), cap,
                                                           C.byref(rows), C.byref(bad)))
        return out[:min(cap, int(rows.value))], int(rows.value), int(bad.value)

    def read_snps_counts_device(self, paths, row_begin: int = 0, max_rows: int = -1, first_slot: int = 0, extra_slots: int = 0):
        """The count columns of several samples' <species>.snps.gz inflated and parsed on the device
        (midas_snps_tableset_read_counts_device) -> MergeTables: table k of `paths` in sample slot first_slot + k, rows
        [row_begin, max_rows) of the SHORTEST table (max_rows < 0: its end), as read_snps_counts.  first_slot / extra_slots: slots in
        front of / behind the tables' for samples the caller fills (MergeTables.set_host).  Raises MidasSnpsError: ERR_UNSUPPORTED
        when a file does not announce its rows, ERR_BAD_LAYOUT (naming the file) when one is corrupt; nothing stays allocated."""
        with _TableSet(self._lib, paths) as ts:
            if (ts.rows < 0).any():
                raise MidasSnpsError(ERR_UNSUPPORTED, "%s: the file does not announce its rows" % paths[int(np.nonzero(ts.rows < 0)[0][0])])
            m = ts.count(row_begin, max_rows)
            tables = MergeTables(self, int(first_slot) + ts.n + int(extra_slots), m)
            stats, ms = np.zeros(8, np.int64), np.zeros(4, np.float32)
            try:
                host_call(self._lib.midas_snps_tableset_read_counts_device, self._h, ts.h, int(row_begin), m, int(first_slot), tables._h,
                          ptr(stats), ptr(ms))
            except MidasSnpsError:
                tables.close()
                raise
            tables.stats = dict(zip(TABLES_READ_STATS, (int(x) for x in stats)))
            tables.ms = dict(zip(TABLES_READ_PHASES, (float(x) for x in ms)))
            return tables

    @staticmethod
    def _merge_inputs(sample_counts, mean_depth, with_matrices: bool):
        """(first arguments after the parameters, output dict, calls [n, 4]) of the four merge_sites forms: sample_counts a
        MergeTables (handle, n, mean_depth) or the list of the samples' arrays (S, n, pointers, mean_depth)."""
        md = np.ascontiguousarray(mean_depth, dtype=np.float64)
        if isinstance(sample_counts, MergeTables):
            n, S = sample_counts.n_sites, sample_counts.n_samples
            assert md.shape == (S,)
            head, keep = (sample_counts._h, n, addr(md)), md
        else:
            S = len(sample_counts)
            arrs = [np.ascontiguousarray(a, dtype=np.uint32) for a in sample_counts]
            n = arrs[0].shape[0]
            assert all(a.shape == (n, 4) for a in arrs)
            head, keep = (S, n, (C.c_void_p * S)(*[a.ctypes.data for a in arrs]), addr(md)), (arrs, md)
        calls = np.empty((n, 4), np.uint8)
        out = dict(major=calls[:, 0], minor=calls[:, 1], snp_type=calls[:, 2], flag=calls[:, 3],
                   count_samples=np.empty(n, np.uint32), pooled=np.empty((n, 4), np.uint64))
        if with_matrices:
            out.update(depth=np.empty((S, n), np.uint32), minor_count=np.empty((S, n), np.uint32))
        # (addr throughout: a species of no sites is merged from, and into, empty arrays)
        return head, out, calls, keep

    def merge_sites(self, prm: "MergeParams", sample_counts, mean_depth):
        """midas_merge_sites(): sample_counts = list of [n_sites,4] uint32 arrays (one per sample), or a MergeTables (the counts
        where the device readers left them: midas_merge_sites_resident).
        -> dict(major, minor, snp_type, flag, count_samples, pooled[n,4] u64, depth[S,n] u32, minor_count[S,n] u32, kernel_ms)"""
        fn = self._lib.midas_merge_sites_resident if isinstance(sample_counts, MergeTables) else self._lib.midas_merge_sites
        head, out, calls, keep = self._merge_inputs(sample_counts, mean_depth, True)
        ms = C.c_float(0)
        st = fn(self._h, C.byref(prm), *head, addr(calls), addr(out['count_samples']), addr(out['pooled']),
                addr(out['depth']), addr(out['minor_count']), C.byref(ms))
        del keep
        self._check(st)
        out['kernel_ms'] = float(ms.value)
        return out

    def merge_sites_tables(self, prm: "MergeParams", sample_counts, mean_depth, freq_path: str, depth_path: str, header_line: str,
                           site_id_base: int = 0):
        """midas_merge_sites_tables(): merge_sites with snps_freq.txt / snps_depth.txt written from the device -- depth and
        minor_count stay there.  -> dict(major, minor, snp_type, flag, count_samples, pooled[n,4] u64, n_keep, kernel_ms,
        format_ms).  sample_counts: the list of arrays, or a MergeTables (midas_merge_sites_tables_resident)."""
        fn = self._lib.midas_merge_sites_tables_resident if isinstance(sample_counts, MergeTables) else self._lib.midas_merge_sites_tables
        head, out, calls, keep = self._merge_inputs(sample_counts, mean_depth, False)
        ms, fms, kept = C.c_float(0), C.c_float(0), C.c_int64(0)
        st = fn(self._h, C.byref(prm), *head, freq_path.encode(), depth_path.encode(), header_line.encode(), int(site_id_base),
                addr(calls), addr(out['count_samples']), addr(out['pooled']), C.byref(kept), C.byref(ms), C.byref(fms))
        del keep
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
        keep = (cl, cp, dp, rd)     # (alive during the call)
        st = self._lib.midas_genes_merge(self._h, S, ptr(n), ptrs(cl), ptrs(cp), ptrs(dp), ptrs(rd), int(n_clusters), float(min_copy),
                                         int(group_samples), cap, C.byref(R), ptr(out['rows']), ptr(out['copy']), ptr(out['depth']),
                                         ptr(out['reads']), ptr(out['state']), C.byref(ms))
        del keep
        self._check(st)
        r = int(R.value)
        res = {k: v[:r] for k, v in out.items()}
        res['kernel_ms'] = float(ms.value)
        return res
