"""snp_pairs.py: the host side.

The reference gives "between-sample heterogeneity" (docs/snp_diversity.md, example 2) as snp_diversity.py --sample_type
pooled-samples: one number for the whole pool.  Which samples differ takes one run per pair with --keep_samples a,b.  Here all
pairs are one device pass (Context.sites_pair_diversity): the rows are parsed once, every (site, sample) cell is flagged once,
and prevalence, pooled frequency, --site_prev, --site_maf and --max_sites are decided per (pair, site).

Contract A, the pooled block: dropping sample1, sample2 and the columns from shared_sites on leaves, for every row, the file
`snp_diversity.py --sample_type pooled-samples --genomic_type genome-wide` writes under the same --seed with exactly the two
samples selected and otherwise the same options (the sample-selection options aside).
Contract B, the shared block, over the pair's retained sites at which both samples are kept: shared_sites, the within-sample
pi_bp of either sample, dxy = the mean of a (1 - b) + b (1 - a), fst = 1 - ((pi_bp_1 + pi_bp_2) / 2) / dxy (Hudson) and
da = dxy - (pi_bp_1 + pi_bp_2) / 2, the divisions in numpy fp64 here.

Stated deviations from the separate runs: a malformed cell, or under --consensus a frequency that is not finite, ends the command
wherever it stands in the rows the site mask spans, even where one pair's own --max_sites run would have stopped before it.
--rand_reads is not offered: each separate run draws numpy's stream from its own start over its own sites.
"""
import random
import sys

import numpy as np

from midas_amd import abi
from midas_amd.analyze import cli, diversity, trees
from midas_amd.analyze import sites as S

HEADER = ['sample1', 'sample2', 'samples'] + diversity.BLOCK_COLUMNS + ['shared_sites', 'pi_bp_1', 'pi_bp_2', 'dxy', 'fst', 'da']


def compute(args, tables, samples, ctx):
    order = list(samples.values())
    mask, n = diversity.site_mask(tables, args)
    flags = (abi.SITES_WEIGHT if args['weight_by_depth'] else 0) | (abi.SITES_ROUND if args['consensus'] else 0)
    try:
        return ctx.sites_pair_diversity(tables.freq_text, tables.depth_text, np.ascontiguousarray(mask[:n], np.uint8), [s.index for s in order],
                                        [s.mean_depth for s in order], int(args['site_depth']), float(args['site_ratio']),
                                        float(args['allele_support']), float(args['site_prev']), float(args['site_maf']),
                                        snp_maf=float(args['snp_maf']), max_sites=-1 if args['max_sites'] == float('inf') else int(args['max_sites']),
                                        flags=flags, group_rows=int(args.get('group_rows', 0) or 0), chunk_bytes=int(args.get('chunk_bytes', 0) or 0),
                                        pair_form=int(args.get('pair_form', 0) or 0))
    except abi.MidasSnpsError as e:
        if getattr(e, 'bad', None):
            S.exit_bad_row(tables, order, e)
        trees._exit_limit(e, len(order))


def shared_block(res, i, j):
    """Contract B for the pairs (i[k], j[k]) -> dict of float arrays pi_bp_1, pi_bp_2, dxy, fst, da (nan where there is none) and
    the bool array `some`: the pair has a shared site."""
    shared = res['shared'][i, j]
    some = shared > 0
    div = np.where(some, shared, 1).astype(np.float64)
    with np.errstate(all='ignore'):
        p1, p2, dxy = res['w1'][i, j] / div, res['w2'][i, j] / div, res['x'][i, j] / div
        w = (p1 + p2) / 2.0
        fst = 1.0 - w / dxy
        da = dxy - w
    nan = lambda v, ok: np.where(ok, v, np.nan)
    return dict(some=some, pi_bp_1=nan(p1, some), pi_bp_2=nan(p2, some), dxy=nan(dxy, some), fst=nan(fst, some & (dxy != 0.0)), da=nan(da, some),
                fst_ok=some & (dxy != 0.0))


def pair_rows(args, names, res):
    """-> the table's rows (lists of cells) below the header, in itertools.combinations order."""
    n = len(names)
    i, j = np.triu_indices(n, 1)
    pooled = diversity.chain_cells(dict(args, sample_type='pooled-samples'), res['pi'][i, j], res['snps'][i, j], res['sites'][i, j])
    sb = shared_block(res, i, j)

    def cells(key, ok):
        out = np.full(i.shape[0], 'NA', object)
        if ok.any():
            out[ok] = abi.format_repr_f64(sb[key][ok])
        return out

    shared = [str(x) for x in res['shared'][i, j].tolist()]
    cols = [cells(k, sb['some']) for k in ('pi_bp_1', 'pi_bp_2', 'dxy')] + [cells('fst', sb['fst_ok']), cells('da', sb['some'])]
    return [[names[a], names[b], '2'] + [pooled[c][k] for c in diversity.BLOCK_COLUMNS] + [shared[k]] + [col[k] for col in cols]
            for k, (a, b) in enumerate(zip(i.tolist(), j.tolist()))]


def da_matrix(names, res):
    """da of every pair, mirrored, with a zero diagonal; negative values stay as they come.  A pair without a shared site has no
    da: the first one in (i, j) order ends the command."""
    n = len(names)
    i, j = np.triu_indices(n, 1)
    sb = shared_block(res, i, j)
    if not sb['some'].all():
        k = int(np.flatnonzero(~sb['some'])[0])
        sys.exit("\nError: the samples %s and %s have no site at which both of them are kept, so no da.\n"
                 "Try a lower --site_depth, or leave out poorly covered samples with --sample_depth or --sample_cov\n" % (names[i[k]], names[j[k]]))
    if not np.isfinite(sb['da']).all():
        k = int(np.flatnonzero(~np.isfinite(sb['da']))[0])
        sys.exit("\nError: da of the samples %s and %s is not a finite number, so no tree\n" % (names[i[k]], names[j[k]]))
    d = np.zeros((n, n), np.float64)
    d[i, j] = sb['da']
    return d + d.T


def write_pairs(path, rows):
    with open(path, 'w') as out:
        out.write(''.join('\t'.join(r) + '\n' for r in [HEADER] + rows))


def run_pipeline(args, make_context=S.device_context):
    """diversity.run_pipeline for every pair at once.  --seed: both global random streams are seeded before anything draws from
    them.  make_context: tests substitute a CPU double of the device."""
    if args.get('seed') is not None:
        np.random.seed(args['seed'])
        random.seed(args['seed'])
    print("\nSelecting subset of samples...")
    tables = S.open_tables(args['indir'])
    samples = S.fetch_samples(tables, args['sample_depth'], args['fract_cov'], args['max_samples'], args['keep_samples'],
                              args['exclude_samples'], args['rand_samples'])
    print(" %s samples selected" % len(samples))
    names = list(samples)
    if len(names) < 2:
        sys.exit("\nError: a pair needs 2 samples; %d selected\n" % len(names))
    if args.get('tree'):
        cli.check_tree_samples(names)
    print("Estimating diversity metrics of %d pairs...\n" % (len(names) * (len(names) - 1) // 2))
    ctx = make_context()
    try:
        res = compute(args, tables, samples, ctx)
        if args.get('tree'):
            res['da'] = da_matrix(names, res)
            try:
                res['tree'] = ctx.nj_tree(res['da'])
            except abi.MidasSnpsError as e:
                trees._exit_limit(e, len(names))
    finally:
        ctx.close()
    write_pairs(args['out'], pair_rows(args, names, res))
    if args.get('tree'):
        with open(args['tree'], 'w') as out:
            out.write(trees.newick(names, res['tree']))
    return res
