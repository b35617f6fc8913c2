"""MI355X-native snp_diversity.py: the host side.

Mirrors scripts/snp_diversity.py: compute_snp_diversity (:182-258) becomes one device call -- the matrices
parsed, every site's samples flagged, pooled and filtered, and pi / snps / sites / depth summed in site order per chain -- and
write_pi (:260-297) formats the chains as str() does.  The sequential rules that need no frequency (--site_list walked with one
cursor, --rand_sites drawn with random.uniform per site that gets past the list) are applied here, as a mask.  --rand_reads
hands numpy's global generator state to the device call, which resamples the reads of every retained variable site from it, and
takes the state back that the reference's loop would have left.
"""
import random
import sys

import numpy as np

from midas_amd import abi
from midas_amd.analyze import sites as S


def site_mask(tables, args):
    """-> (mask [n] bool, rows the reference reads).  --site_list: a listed id that is absent or out of order blocks every id
    after it, and the loop ends at the first row after the list is used up.  --rand_sites: one draw per site past the list."""
    n = tables.n_sites
    mask = S.info_mask(tables, args['locus_type'], args['site_type'])
    if args['site_list']:
        listed = S.read_site_list(args['site_list'])
        ids = tables.strings('site_id')
        on = np.zeros(n, bool)
        cursor = 0
        for i in range(n):
            if cursor >= len(listed):
                n = i + 1
                break
            if ids[i] == listed[cursor]:
                on[i] = True
                cursor += 1
        mask &= on
    if args['rand_sites']:
        candidates = np.flatnonzero(on[:n]) if args['site_list'] else range(n)
        drop = [i for i in candidates if random.uniform(0, 1) > args['rand_sites']]
        mask[np.array(drop, np.int64)] = False
    return mask, n


def compute(args, tables, samples, ctx):
    pooled, per_gene = args['sample_type'] == 'pooled-samples', args['genomic_type'] == 'per-gene'
    flags = abi.SITES_SUMS | (abi.SITES_POOLED if pooled else 0) | (abi.SITES_PER_GENE if per_gene else 0) | \
        (abi.SITES_WEIGHT if args['weight_by_depth'] else 0) | (abi.SITES_ROUND if args['consensus'] else 0)
    mask, n = site_mask(tables, args)
    kw = {}
    if args.get('rand_reads'):
        # numpy's global stream as it stands when the site loop begins: the device continues it, and the loop's end state goes back
        kw = dict(rand_reads=int(args['rand_reads']), replace_reads=bool(args['replace_reads']), np_state=np.random.get_state(),
                  draw_chunk=int(args.get('draw_chunk', 0) or 0))
    res = S.scan(ctx, tables, samples, mask, n, args, flags, snp_maf=float(args['snp_maf']),
                 site_gene=tables.gene[:n] if per_gene else None, n_genes=tables.n_genes, **kw)
    if kw:
        np.random.set_state(res['np_state'])
    if res['no_gene']:
        sys.exit("\nError: %s/snps_info.txt: %d retained sites have no gene_id (--genomic_type per-gene)\n" % (tables.dir, res['no_gene']))
    return res


def write_pi(args, tables, samples, res):
    """write_pi: one row per chain, every number as str() prints it.  pi is the int 0 until a float is added to it: it prints
    '0' for a chain without a site, and for every per-sample chain under --consensus, whose terms are all the int 0."""
    pooled, per_gene = args['sample_type'] == 'pooled-samples', args['genomic_type'] == 'per-gene'
    sites, snps = res['sites'].ravel(), res['snps'].ravel()
    some = sites > 0
    div = np.where(some, sites, 1).astype(np.float64)
    fmt = lambda v: np.array(abi.format_repr_f64(v), object)
    saw_float = some & (pooled or not args['consensus'])
    pi = np.where(saw_float, fmt(res['pi'].ravel()), '0')
    snps_kb = np.where(some, fmt((1000 * snps).astype(np.float64) / div), 'NA')
    pi_bp = np.where(some, fmt(np.where(saw_float, res['pi'].ravel(), 0.0) / div), 'NA')
    genes = tables.strings('gene_id') if per_gene else [None]
    G = len(genes)
    lines = []
    if pooled:
        lines.append((['gene_id'] if per_gene else []) + ['samples', 'sites', 'snps', 'pi', 'snps_kb', 'pi_bp'])
        for g in range(G):
            lines.append(([genes[g]] if per_gene else []) + [str(len(samples)), str(sites[g]), str(snps[g]), pi[g], snps_kb[g], pi_bp[g]])
    else:
        depth = res['depth'].ravel()
        lines.append(['sample_id'] + (['gene_id'] if per_gene else []) + ['depth', 'sites', 'snps', 'pi', 'snps_kb', 'pi_bp'])
        for k, s in enumerate(samples.values()):
            for g in range(G):
                c = k * G + g
                lines.append([s.id] + ([genes[g]] if per_gene else []) + [str(depth[c]), str(sites[c]), str(snps[c]), pi[c], snps_kb[c], pi_bp[c]])
    with open(args['out'], 'w') as out:
        out.write(''.join('\t'.join(r) + '\n' for r in lines))


def run_pipeline(args, make_context=S.device_context):
    """scripts/snp_diversity.py:299-315.  make_context: tests substitute a CPU double of the device.  --seed: both global random
    streams are seeded before anything draws from them."""
    if args.get('seed') is not None:
        np.random.seed(args['seed'])
        random.seed(args['seed'])
    print("\nSelecting subset of samples...")
    tables = S.open_tables(args['indir'])
    samples = S.fetch_samples(tables, args['sample_depth'], args['fract_cov'], args['max_samples'], args['keep_samples'],
                              args['exclude_samples'], args['rand_samples'])
    print(" %s samples selected" % len(samples))
    print("Estimating diversity metrics...\n")
    ctx = make_context()
    try:
        res = compute(args, tables, samples, ctx)
    finally:
        ctx.close()
    write_pi(args, tables, samples, res)
    return res
