"""MI355X-native snp_trees.py: the host side.

The workflow of docs/snp_trees.md ("Core-Genome Phylogenetic Trees") in one command: the consensus calls of call_consensus.py,
the distances between them and a neighbour-joining tree, without a FASTA or a tree builder in between.  The device walks the two
matrices once and returns, for every pair of samples, the sites called in both and those of them where the two calls differ
(Context.sites_consensus_pairs); the division is numpy's here; the tree is the device's again (Context.nj_tree), and the Newick
text and the pair table are put together here.  Unlike call_consensus.py, --keep_samples and --exclude_samples are applied.

A difference is one of allele role, minor against major: it is the difference of the letters call_consensus.py writes wherever
a site's two allele columns differ, which is everywhere in a directory `merge_midas.py snps` wrote.
"""
import sys

import numpy as np

from midas_amd import abi
from midas_amd.analyze import cli
from midas_amd.analyze import sites as S

PAIRS_HEADER = ['sample1', 'sample2', 'sites', 'mismatches', 'distance']


def site_mask(args, tables):
    """-> (mask, flags): call_consensus.py's -- a --site_list is a set that replaces the site filters."""
    if args['site_list']:
        listed = set(S.read_site_list(args['site_list']))
        return np.fromiter((i in listed for i in tables.strings('site_id')), bool, tables.n_sites), abi.SITES_MASK_ONLY
    return S.info_mask(tables, args['locus_type'], args['site_type']), 0


def distances(order, both, diff):
    """d[i][j] = diff / both, one IEEE division a pair, mirrored, with a zero diagonal.  A pair without a site called in both
    samples has no distance: the first one in (i, j) order ends the command."""
    n = len(order)
    upper = np.triu(np.ones((n, n), bool), 1)
    empty = np.argwhere(upper & (both == 0))
    if empty.shape[0]:
        i, j = (int(x) for x in empty[0])
        sys.exit("\nError: the samples %s and %s have no site called in both of them, so no distance.\n"
                 "Try a higher --site_prev, or leave out poorly covered samples with --sample_depth or --sample_cov\n" % (order[i].id, order[j].id))
    d = np.zeros((n, n), np.float64)
    d[upper] = diff[upper].astype(np.float64) / both[upper].astype(np.float64)
    return d + d.T


def newick(names, tree):
    """(X_a:la,X_b:lb) for every join, in slot a from then on; the last three slots are the root's children."""
    node = list(names)
    text = iter(abi.format_repr_f64(np.concatenate([np.asarray(tree['len'], np.float64).ravel(), np.asarray(tree['last_len'], np.float64)])))
    for a, b in np.asarray(tree['join']).tolist():
        node[a] = '(%s:%s,%s:%s)' % (node[a], next(text), node[b], next(text))
    return '(%s);\n' % ','.join('%s:%s' % (node[k], next(text)) for k in np.asarray(tree['last']).tolist())


def write_pairs(path, names, both, diff, d):
    n = len(names)
    i, j = np.triu_indices(n, 1)                    # (itertools.combinations order)
    text = abi.format_repr_f64(d[i, j])
    with open(path, 'w') as out:
        out.write('\t'.join(PAIRS_HEADER) + '\n')
        out.write(''.join('%s\t%s\t%d\t%d\t%s\n' % (names[a], names[b], s, m, t)
                          for a, b, s, m, t in zip(i.tolist(), j.tolist(), both[i, j].tolist(), diff[i, j].tolist(), text)))


def _exit_limit(e, n):
    if getattr(e, 'limit', None) is not None:
        sys.exit("\nError: %d samples selected, but the distance matrix of at most %d samples fits the free device memory.\n"
                 "Select fewer with --max_samples, --sample_depth, --sample_cov or --exclude_samples\n" % (n, e.limit))
    sys.exit("\nError: %s\n" % e.message)


def compute(args, tables, samples, ctx):
    order = list(samples.values())
    mask, flags = site_mask(args, tables)
    try:
        res = ctx.sites_consensus_pairs(tables.freq_text, tables.depth_text, np.ascontiguousarray(mask, np.uint8), [s.index for s in order],
                                        [s.mean_depth for s in order], int(args['site_depth']), float(args['site_ratio']),
                                        float(args['allele_support']), float(args['site_prev']), float(args['site_maf']),
                                        max_sites=-1 if args['max_sites'] == float('inf') else int(args['max_sites']), flags=flags,
                                        group_rows=int(args.get('group_rows', 0) or 0), chunk_bytes=int(args.get('chunk_bytes', 0) or 0))
    except abi.MidasSnpsError as e:
        if getattr(e, 'bad', None):
            S.exit_bad_row(tables, order, e)
        _exit_limit(e, len(order))
    res['dist'] = distances(order, res['both'], res['diff'])
    try:
        res['tree'] = ctx.nj_tree(res['dist'])
    except abi.MidasSnpsError as e:
        _exit_limit(e, len(order))
    return res


def run_pipeline(args, make_context=S.device_context):
    """make_context: tests substitute a CPU double of the device."""
    tables = S.open_tables(args['indir'])
    samples = S.fetch_samples(tables, args['sample_depth'], args['fract_cov'], args['max_samples'], args['keep_samples'],
                              args['exclude_samples'])
    cli.check_tree_samples(list(samples))
    ctx = make_context()
    try:
        res = compute(args, tables, samples, ctx)
    finally:
        ctx.close()
    names = list(samples)
    with open(args['out'], 'w') as out:
        out.write(newick(names, res['tree']))
    if args.get('dist'):
        write_pairs(args['dist'], names, res['both'], res['diff'], res['dist'])
    return res
