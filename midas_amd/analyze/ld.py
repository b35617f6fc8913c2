"""MI355X-native snp_ld.py: the host side.

Linkage disequilibrium between pairs of sites of one merged species directory, by distance.  The host
gives every row of snps_info.txt a position key (contig index x 2^40 + ref_pos), checks that the keys of the rows it passes on
ascend, and forms the site mask of call_consensus.py; the device walks the two matrices once, keeps the consensus calls of the
retained sites resident and returns, per distance bin, the pairs of sites, the informative ones and three ordered fp64 sums
(Context.sites_ld).  The two divisions per bin are numpy's here, and the table is written here.
"""
import os
import sys

import numpy as np

from midas_amd import abi
from midas_amd.analyze import cli
from midas_amd.analyze import sites as S
from midas_amd.analyze import trees

HEADER = ['bin_start', 'bin_end', 'site_pairs', 'ld_pairs', 'r2', 'sigma2_d']
KEY_SHIFT = 40                  # key = contig index << 40 | ref_pos


def site_keys(tables, mask):
    """-> int64 [n_sites]: contig index * 2^40 + ref_pos.  Over the rows of the mask the keys must ascend strictly (the sites
    of a contig together, in the order of their positions): the first row that breaks it ends the command."""
    try:
        contig, pos = tables.contig, tables.ref_pos
    except abi.MidasSnpsError as e:
        sys.exit("\nError: %s\n" % e.message)
    info = os.path.join(tables.dir, 'snps_info.txt')
    on = np.flatnonzero(mask)
    bad = on[(pos[on] < 0) | (pos[on] >= 1 << KEY_SHIFT)]
    if bad.shape[0]:
        sys.exit("\nError: %s, line %d: ref_pos must be between 0 and 2^40 - 1\n" % (info, int(bad[0]) + 2))
    key = contig.astype(np.int64) * (1 << KEY_SHIFT) + pos
    back = np.flatnonzero(key[on][1:] <= key[on][:-1])
    if back.shape[0]:
        sys.exit("\nError: %s, line %d: the site does not lie behind the one before it (line %d); the sites of a contig must stand\n"
                 "together, in ascending ref_pos\n" % (info, int(on[back[0] + 1]) + 2, int(on[back[0]]) + 2))
    return key


def bin_bounds(max_dist, bin_width):
    """-> (first, last distance) of every bin."""
    n_bins = -(-max_dist // bin_width)
    start = np.arange(n_bins, dtype=np.int64) * bin_width + 1
    return start, np.minimum(start + bin_width - 1, max_dist)


def ratios(res):
    """r2 = sum_r2 / ld_pairs, sigma2_d = sum_d2 / sum_het: one numpy division each; nan where the bin has no informative pair."""
    pairs = res['pairs']
    with np.errstate(divide='ignore', invalid='ignore'):
        r2 = np.asarray(res['sum_r2'], np.float64) / pairs.astype(np.float64)
        sigma = np.asarray(res['sum_d2'], np.float64) / np.asarray(res['sum_het'], np.float64)
    r2[pairs == 0] = np.nan
    sigma[pairs == 0] = np.nan
    return r2, sigma


def write_table(path, max_dist, bin_width, res):
    start, end = bin_bounds(max_dist, bin_width)
    r2, sigma = ratios(res)
    on = res['pairs'] > 0
    text = iter(abi.format_repr_f64(np.stack([r2[on], sigma[on]], axis=1).ravel()))
    with open(path, 'w') as out:
        out.write('\t'.join(HEADER) + '\n')
        out.write(''.join('%d\t%d\t%d\t%d\t%s\t%s\n' % ((a, b, w, p) + ((next(text), next(text)) if p else ('NA', 'NA')))
                          for a, b, w, p in zip(start.tolist(), end.tolist(), res['window'].tolist(), res['pairs'].tolist())))


def compute(args, tables, samples, ctx):
    order = list(samples.values())
    mask, flags = trees.site_mask(args, tables)
    key = site_keys(tables, mask)
    if args['within'] == 'gene':
        flags |= abi.SITES_LD_SAME_GENE
    try:
        return ctx.sites_ld(tables.freq_text, tables.depth_text, np.ascontiguousarray(mask, np.uint8), [s.index for s in order],
                            [s.mean_depth for s in order], key, tables.gene, int(args['site_depth']), float(args['site_ratio']),
                            float(args['allele_support']), float(args['site_prev']), float(args['site_maf']), max_dist=int(args['max_dist']),
                            bin_width=int(args['bin_width']), min_samples=int(args['min_samples']),
                            max_sites=-1 if args['max_sites'] == float('inf') else int(args['max_sites']), flags=flags,
                            group_rows=int(args.get('group_rows', 0) or 0), chunk_bytes=int(args.get('chunk_bytes', 0) or 0),
                            anchor_chunk=int(args.get('anchor_chunk', 0) or 0))
    except abi.MidasSnpsError as e:
        if getattr(e, 'bad', None):
            S.exit_bad_row(tables, order, e)
        if getattr(e, 'limit', None) is not None:
            sys.exit("\nError: %d sites pass the site filters that need no frequency, but the calls of at most %d sites of %d samples fit\n"
                     "the free device memory.  Use --max_sites, --locus_type or --site_list, or fewer samples\n"
                     % (int(np.count_nonzero(mask)), e.limit, len(order)))
        sys.exit("\nError: %s\n" % e.message)


def run_pipeline(args, make_context=S.device_context):
    """make_context: tests substitute a CPU double of the device."""
    tables = S.open_tables(args['indir'])
    samples = S.fetch_samples(tables, args['sample_depth'], args['fract_cov'], args['max_samples'], args['keep_samples'],
                              args['exclude_samples'])
    ctx = make_context()
    try:
        res = compute(args, tables, samples, ctx)
    finally:
        ctx.close()
    write_table(args['out'], int(args['max_dist']), int(args['bin_width']), res)
    return res
