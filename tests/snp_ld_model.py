"""A sequential model of snp_ld.py: the consensus calls of the retained sites by a restatement of the rule
of call_consensus.py, the pairs of sites inside the distance window, the four counts of a pair as Python integers over bit
masks, the terms one fp64 operation at a time, the two serial levels of the sums, the divisions and the table.  The host tests
inject ModelContext in place of the device; the GPU tests compare the device call and the script's file with it.  Also here:
the helpers that rewrite columns of a synthetic species directory's snps_info.txt (positions, genes)."""
import os

import numpy as np

from midas_amd import abi
from midas_amd.analyze import cli, sites, trees
from tests import analyze_model

KEY_SHIFT = 40


# ---- the calls ------------------------------------------------------------------------------------------------------------------
def consensus_calls(freq_text, depth_text, site_mask, sample_col, mean_depth, site_depth, site_ratio, allele_support, site_prev, site_maf,
                    max_sites=-1, flags=0):
    """-> dict(rows = the retained rows, called / minor bool [S, retained], n_sites, n_kept, side_freq, side_depth).  Row by row as
    the reference reads them: the cells of the selected samples (the frequency before the depth, a sample after the other), then
    the stop of --max_sites, then the samples' flags, the site's prevalence and pooled frequency, the site's filters."""
    frows, drows = analyze_model._rows(freq_text), analyze_model._rows(depth_text)
    mask = np.asarray(site_mask, np.uint8)
    cols = [int(c) for c in sample_col]
    mean = np.array([float(x) for x in mean_depth], np.float64)
    S = len(cols)
    mask_only = bool(flags & abi.SITES_MASK_ONLY)
    n = min(int(mask.shape[0]), len(frows), len(drows))
    rows, called, minor = [], [], []
    side = [0, 0]
    n_read = 0
    stopped = False
    for i in range(n):
        n_read = i + 1
        fr, dr = frows[i][1:], drows[i][1:]
        f, d = np.zeros(S, np.float64), np.zeros(S, np.int64)
        for s in range(S):
            for m, (row, conv, fast, out) in enumerate(((fr, float, analyze_model.is_fast_float, f), (dr, int, analyze_model.is_fast_int, d))):
                if cols[s] >= len(row):
                    raise analyze_model.BadCell((m + 1, i, -1), "%s matrix, data row %d: fewer columns than the samples in use" % (('freq', 'depth')[m], i))
                cell = row[cols[s]]
                side[m] += 0 if fast(cell) else 1
                try:
                    out[s] = conv(cell)
                except ValueError:
                    raise analyze_model.BadCell((m + 1, i, s), "%s matrix, data row %d, sample %d: not a number" % (('freq', 'depth')[m], i, s))
        if max_sites >= 0 and len(rows) >= max_sites:
            stopped = True
            break
        with np.errstate(all='ignore'):
            support = np.where((1.0 - f) > f, 1.0 - f, f)               # Python's max(f, 1 - f)
            keep = ~(d < site_depth) & ~(d.astype(np.float64) / mean > site_ratio) & ~(support < allele_support)
        count = int(keep.sum())
        retained = bool(mask[i])
        if not mask_only:
            if site_prev and float(count) / S < max(1e-6, site_prev):
                retained = False
            if site_maf:
                pooled = float(np.add.reduce(f[keep])) / count if count else 0.0      # numpy's mean over the kept frequencies
                if pooled < site_maf:
                    retained = False
        if not retained:
            continue
        rows.append(i)
        c = keep & (d != 0)
        called.append(c)
        minor.append(c & (f >= 0.5))
    shape = (S, len(rows))
    return dict(rows=np.array(rows, np.int64), called=np.array(called, bool).reshape(shape[::-1]).T, minor=np.array(minor, bool).reshape(shape[::-1]).T,
                n_sites=n_read if stopped else n, n_kept=len(rows), side_freq=side[0], side_depth=side[1])


def _bits(column):
    return sum(1 << s for s in np.flatnonzero(column).tolist())


def _popc(x):
    return bin(x).count('1')


def ld_sums(called, minor, key, gene, max_dist, bin_width, min_samples, same_gene):
    """The definition over the retained sites' calls [S, M], keys [M] and genes [M] -> dict(window, pairs, sum_r2, sum_d2, sum_het,
    n_hist = {n: pairs of sites that are informative but for --min_samples}, r2_values = the distinct r2)."""
    M = int(called.shape[1])
    n_bins = -(-max_dist // bin_width)
    C = [_bits(called[:, k]) for k in range(M)]
    Mi = [_bits(minor[:, k]) for k in range(M)]
    key = [int(x) for x in key]
    window, pairs = np.zeros(n_bins, np.int64), np.zeros(n_bins, np.int64)
    total = np.zeros((3, n_bins), np.float64)             # +0.0
    n_hist, r2_values = {}, set()
    for a in range(M):
        p = np.zeros((3, n_bins), np.float64)             # p_x[a][bin], +0.0
        for b in range(a + 1, M):
            dist = key[b] - key[a]
            assert dist >= 1
            if dist > max_dist:
                break
            if same_gene and not (gene[a] >= 0 and gene[a] == gene[b]):
                continue
            beta = (dist - 1) // bin_width
            window[beta] += 1
            both = C[a] & C[b]
            n, na, nb, nab = _popc(both), _popc(both & Mi[a]), _popc(both & Mi[b]), _popc(both & Mi[a] & Mi[b])
            if not (0 < na < n and 0 < nb < n):
                continue
            n_hist[n] = n_hist.get(n, 0) + 1
            if n < min_samples:
                continue
            Dn = n * nab - na * nb
            ha, hb = na * (n - na), nb * (n - nb)
            num = float(Dn) * float(Dn)
            den = float(ha) * float(hb)
            r2 = num / den
            n2 = float(n * n)
            n4 = n2 * n2
            d2 = num / n4
            het = den / n4
            pairs[beta] += 1
            p[0, beta] = p[0, beta] + r2                  # one add a partner, in ascending b
            p[1, beta] = p[1, beta] + d2
            p[2, beta] = p[2, beta] + het
            r2_values.add(r2)
        total = total + p                                 # one add an anchor and bin, in ascending a (elementwise fp64)
    return dict(window=window, pairs=pairs, sum_r2=total[0].copy(), sum_d2=total[1].copy(), sum_het=total[2].copy(), n_hist=n_hist,
                r2_values=r2_values)


def sites_ld(freq_text, depth_text, site_mask, sample_col, mean_depth, site_key, site_gene, site_depth, site_ratio, allele_support,
             site_prev, site_maf, max_dist=1000, bin_width=10, min_samples=4, max_sites=-1, flags=0, group_rows=0, chunk_bytes=0,
             anchor_chunk=0):
    """Context.sites_ld by the model."""
    calls = consensus_calls(freq_text, depth_text, site_mask, sample_col, mean_depth, site_depth, site_ratio, allele_support, site_prev,
                            site_maf, max_sites=max_sites, flags=flags)
    rows = calls['rows']
    key = np.asarray(site_key, np.int64)[rows]
    gene = np.asarray(site_gene, np.int64)[rows] if site_gene is not None else np.zeros(rows.shape[0], np.int64)
    out = ld_sums(calls['called'], calls['minor'], key, gene, int(max_dist), int(bin_width), int(min_samples), bool(flags & abi.SITES_LD_SAME_GENE))
    out.update(rows=rows, key=key, n_sites=calls['n_sites'], n_kept=calls['n_kept'], side_freq=calls['side_freq'], side_depth=calls['side_depth'],
               pairs_visited=int(out['window'].sum()))
    return out


class ModelContext:
    """Stands in for abi.Context in ld.run_pipeline.  site_limit: what the device's free memory would hold."""

    def __init__(self, site_limit=1 << 40):
        self.site_limit = site_limit

    def sites_ld(self, freq_text, depth_text, site_mask, *a, **kw):
        if int(np.count_nonzero(site_mask)) > self.site_limit:
            e = abi.MidasSnpsError(abi.ERR_OUT_OF_MEMORY, "the planes of at most %d sites fit the free device memory" % self.site_limit)
            e.bad, e.limit = None, self.site_limit
            raise e
        try:
            return sites_ld(freq_text, depth_text, site_mask, *a, **kw)
        except analyze_model.BadCell as e:
            e.limit = None
            raise

    def close(self):
        pass


# ---- the host side ----------------------------------------------------------------------------------------------------------------
def read_info_columns(indir, names):
    with open(os.path.join(indir, 'snps_info.txt')) as f:
        lines = [ln for ln in f.read().split('\n') if ln]
    header = lines[0].split('\t')
    at = [header.index(name) for name in names]
    return [[ln.split('\t')[k] for ln in lines[1:]] for k in at]


def info_keys(indir):
    """contig index * 2^40 + ref_pos of every row of snps_info.txt, read here in Python."""
    ref_id, ref_pos = read_info_columns(indir, ['ref_id', 'ref_pos'])
    index = {}
    return np.array([(index.setdefault(c, len(index)) << KEY_SHIFT) + int(p) for c, p in zip(ref_id, ref_pos)], np.int64)


def table(max_dist, bin_width, res):
    rows = ['\t'.join(['bin_start', 'bin_end', 'site_pairs', 'ld_pairs', 'r2', 'sigma2_d'])]
    for k in range(res['window'].shape[0]):
        w, p = int(res['window'][k]), int(res['pairs'][k])
        r2 = repr(float(res['sum_r2'][k]) / float(p)) if p else 'NA'
        sigma = repr(float(res['sum_d2'][k]) / float(res['sum_het'][k])) if p else 'NA'
        rows.append('%d\t%d\t%d\t%d\t%s\t%s' % (k * bin_width + 1, min((k + 1) * bin_width, max_dist), w, p, r2, sigma))
    return '\n'.join(rows) + '\n'


def expected_file(argv):
    """-> (the text `snp_ld.py argv` writes, the model's result), by this model; the argument parser, the sample selection and
    the site mask are the command's own."""
    args = cli.ld_arguments(argv)
    tables = sites.open_tables(args['indir'])
    samples = sites.fetch_samples(tables, args['sample_depth'], args['fract_cov'], args['max_samples'], args['keep_samples'],
                                  args['exclude_samples'])
    order = list(samples.values())
    mask, flags = trees.site_mask(args, tables)
    if args['within'] == 'gene':
        flags |= abi.SITES_LD_SAME_GENE
    res = sites_ld(tables.freq_text, tables.depth_text, np.ascontiguousarray(mask, np.uint8), [s.index for s in order],
                   [s.mean_depth for s in order], info_keys(args['indir']), np.asarray(tables.gene), int(args['site_depth']), float(args['site_ratio']),
                   float(args['allele_support']), float(args['site_prev']), float(args['site_maf']), max_dist=args['max_dist'],
                   bin_width=args['bin_width'], min_samples=args['min_samples'],
                   max_sites=-1 if args['max_sites'] == float('inf') else int(args['max_sites']), flags=flags)
    return table(args['max_dist'], args['bin_width'], res), res


def means_something(res):
    """What every comparison asserts of the model's result first: several bins with informative pairs, a bin where some pairs
    are informative and some are not, at least two distinct r2."""
    return int((res['pairs'] > 0).sum()) >= 3 and bool(((res['pairs'] > 0) & (res['pairs'] < res['window'])).any()) and len(res['r2_values']) >= 2


# ---- test inputs ------------------------------------------------------------------------------------------------------------------
def rewrite_info(indir, columns):
    """columns {name: one string per data row}: those columns of snps_info.txt are replaced, the others stay."""
    path = os.path.join(indir, 'snps_info.txt')
    with open(path) as f:
        lines = f.read().split('\n')
    header = lines[0].split('\t')
    at = {name: header.index(name) for name in columns}
    r = 0
    for k in range(1, len(lines)):
        if not lines[k]:
            continue
        cells = lines[k].split('\t')
        for name, values in columns.items():
            cells[at[name]] = str(values[r])
        lines[k] = '\t'.join(cells)
        r += 1
    assert all(len(v) == r for v in columns.values())
    with open(path, 'w') as f:
        f.write('\n'.join(lines))


def spread_positions(n_rows, retained, max_dist, seed=0):
    """-> (ref_id, ref_pos) per row, laid out around the rows a filter retains (`retained`, ascending):
      contig_a   the first half of the rows: a run of consecutive positions, then steps of 1..3 bases with two wider steps placed
                 so that two neighbouring RETAINED sites lie exactly max_dist and max_dist + 1 apart;
      contig_b   one row, a retained one;
      contig_c   the rest: steps of 1..5 with jumps past the window now and then, and consecutive positions to the last row.
    Positions restart at each contig; within a contig they ascend strictly."""
    rng = np.random.default_rng(seed)
    retained = np.asarray(retained)
    step = np.ones(n_rows, np.int64)
    half = n_rows // 2
    single = int(retained[np.searchsorted(retained, half)])             # contig_b
    quarter = n_rows // 4
    step[quarter:single] = rng.integers(1, 4, single - quarter)
    for target, gap in ((quarter + (single - quarter) // 3, max_dist), (quarter + 2 * (single - quarter) // 3, max_dist + 1)):
        j = int(np.searchsorted(retained, target))
        ka, kb = int(retained[j]), int(retained[j + 1])
        step[ka + 1:kb + 1] = 1
        step[kb] = gap - (kb - ka - 1)
        assert quarter < ka and kb < single and step[kb] >= 1
    rest = np.arange(single + 1, n_rows)
    step[rest] = rng.integers(1, 6, rest.shape[0])
    step[rest[rng.random(rest.shape[0]) < 0.01]] = max_dist + 7
    step[n_rows - 200:] = 1
    ref_id = np.where(np.arange(n_rows) < single, 'contig_a', np.where(np.arange(n_rows) == single, 'contig_b', 'contig_c'))
    pos = np.zeros(n_rows, np.int64)
    for lo, hi, first in ((0, single, 1000), (single, single + 1, 5), (single + 1, n_rows, 17)):
        pos[lo:hi] = first + np.cumsum(step[lo:hi]) - step[lo]
    return ref_id.tolist(), pos.tolist()


def gene_runs(n_rows, run=30, between=10):
    """-> (locus_type, gene_id) per row: genes of `run` rows with `between` rows outside any gene after each."""
    k = np.arange(n_rows)
    inside = k % (run + between) < run
    return (np.where(inside, 'CDS', 'IGR').tolist(), ['gene_%05d' % (i // (run + between)) if on else '' for i, on in zip(k.tolist(), inside.tolist())])
