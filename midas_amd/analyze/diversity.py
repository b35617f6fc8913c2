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


def restrict_mask(tables, args, mask):
    """mask [n] bool (what the info table decides) with --site_list and --rand_sites applied -> (mask, rows the reference reads).
    --site_list: a listed id that is absent or out of order blocks every id after it, and the loop ends at the first row after
    the list is used up.  --rand_sites: one draw per site past the list, whatever the mask holds there (snp_pnps.py and the two
    snp_diversity.py runs it stands for drop the same sites under one seed)."""
    n = tables.n_sites
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


def site_mask(tables, args):
    """-> (mask [n] bool, rows the reference reads): --locus_type / --site_type, then restrict_mask."""
    return restrict_mask(tables, args, S.info_mask(tables, args['locus_type'], args['site_type']))


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


def chain_cells(args, pi, snps, sites, depth=None):
    """The cells of write_pi's columns for every chain of one block of sums (arrays of one shape, read flat), every number as
    str() prints it -> dict of str arrays: sites, snps, pi, snps_kb, pi_bp and (per-sample) depth; and pi_bp_value, the doubles
    whose repr pi_bp holds (nan where it is NA).  pi is the int 0 until a float is added to it: it prints '0' for a chain
    without a site, and for every per-sample chain under --consensus, whose terms are all the int 0."""
    pooled = args['sample_type'] == 'pooled-samples'
    pi, sites, snps = pi.ravel(), sites.ravel(), snps.ravel()
    some = sites > 0
    div = np.where(some, sites, 1).astype(np.float64)
    fmt = lambda v: np.array(abi.format_repr_f64(v), object)
    saw_float = some & (pooled or not args['consensus'])
    pi_bp_value = np.where(saw_float, pi, 0.0) / div
    cells = dict(sites=np.array([str(x) for x in sites], object), snps=np.array([str(x) for x in snps], object),
                 pi=np.where(saw_float, fmt(pi), '0'), snps_kb=np.where(some, fmt((1000 * snps).astype(np.float64) / div), 'NA'),
                 pi_bp=np.where(some, fmt(pi_bp_value), 'NA'), pi_bp_value=np.where(some, pi_bp_value, np.nan))
    if not pooled:
        cells['depth'] = np.array([str(x) for x in depth.ravel()], object)
    return cells


BLOCK_COLUMNS = ['sites', 'snps', 'pi', 'snps_kb', 'pi_bp']


def write_chains(args, tables, samples, blocks, extra=None):
    """One row per chain: the sample id (per-sample), the gene id (per-gene), the pool's sample count (pooled), then per block
    (suffix, chain_cells) its columns -- depth first for per-sample chains -- and then the extra (name, cells) column."""
    pooled, per_gene = args['sample_type'] == 'pooled-samples', args['genomic_type'] == 'per-gene'
    genes = tables.strings('gene_id') if per_gene else [None]
    G = len(genes)
    names = ([] if pooled else ['depth']) + BLOCK_COLUMNS
    header = (['gene_id'] if per_gene else []) + (['samples'] if pooled else []) + [n + suffix for suffix, _ in blocks for n in names] + \
        ([extra[0]] if extra else [])
    lines = [header if pooled else ['sample_id'] + header]
    for k, s in enumerate([None] if pooled else samples.values()):
        for g in range(G):
            c = k * G + g
            lines.append(([] if pooled else [s.id]) + ([genes[g]] if per_gene else []) + ([str(len(samples))] if pooled else []) +
                         [cells[n][c] for _, cells in blocks for n in names] + ([extra[1][c]] if extra else []))
    with open(args['out'], 'w') as out:
        out.write(''.join('\t'.join(r) + '\n' for r in lines))


def write_pi(args, tables, samples, res):
    """write_pi: one row per chain, every number as str() prints it."""
    write_chains(args, tables, samples, [('', chain_cells(args, res['pi'], res['snps'], res['sites'], res.get('depth')))])


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
