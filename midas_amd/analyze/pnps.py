"""snp_pnps.py: the host side.

The reference documents pN/pS as a workflow (docs/snp_diversity.md, examples 5 and 6): snp_diversity.py once with --locus_type
CDS --site_type 1D, once with --site_type 4D, and the ratio of the two pi_bp.  Here both runs are one device pass
(Context.sites_scan_classes): the rows are parsed once, every site is decided once, and the ordered sums run once per class,
side by side.  Class 0 (N) holds the CDS sites of type 1D, class 1 (S) those of type 4D.

The contract: for each class, dropping the other class's columns and pnps and stripping the _<class> suffix gives the file
snp_diversity.py --locus_type CDS --site_type <class> --seed <same> writes, byte for byte, for every option combination
without --max_sites.  --max_sites N keeps the first N retained sites of both classes together (each separate run would stop at
its own N-th site).  --rand_reads is not offered: the two separate runs draw numpy's stream over different site sets, so no
single pass equals both.
"""
import random
import sys

import numpy as np

from midas_amd import abi
from midas_amd.analyze import diversity
from midas_amd.analyze import sites as S

CLASSES = ('1D', '4D')


def class_mask(tables, args):
    """-> (mask [n] bool, class [n] uint8, rows the reference reads): CDS sites of type 1D (class 0) or 4D (class 1), then
    --site_list and --rand_sites as snp_diversity.py applies them."""
    site_class = np.zeros(tables.n_sites, np.uint8)
    member = np.zeros(tables.n_sites, bool)
    for c, name in enumerate(CLASSES):
        of_class = tables.equals('site_type', name)
        site_class[of_class] = c
        member |= of_class
    mask, n = diversity.restrict_mask(tables, args, S.info_mask(tables, 'CDS', None) & member)
    return mask, site_class, n


def compute(args, tables, samples, ctx):
    pooled, per_gene = args['sample_type'] == 'pooled-samples', args['genomic_type'] == 'per-gene'
    flags = abi.SITES_SUMS | (abi.SITES_POOLED if pooled else 0) | (abi.SITES_PER_GENE if per_gene else 0) | \
        (abi.SITES_WEIGHT if args['weight_by_depth'] else 0) | (abi.SITES_ROUND if args['consensus'] else 0)
    mask, site_class, n = class_mask(tables, args)
    res = S.scan(ctx, tables, samples, mask, n, args, flags, classes=(site_class, len(CLASSES)), snp_maf=float(args['snp_maf']),
                 site_gene=tables.gene[:n] if per_gene else None, n_genes=tables.n_genes)
    if res['no_gene']:
        sys.exit("\nError: %s/snps_info.txt: %d retained sites have no gene_id (--genomic_type per-gene)\n" % (tables.dir, res['no_gene']))
    return res


def ratio_cells(n_cells, s_cells):
    """pnps per chain: pi_bp_1D / pi_bp_4D, one division of the two doubles whose repr is printed; NA where either is NA or the
    divisor is 0.0."""
    a, b = n_cells['pi_bp_value'], s_cells['pi_bp_value']
    ok = ~np.isnan(a) & ~np.isnan(b) & (b != 0.0)
    out = np.full(a.shape[0], 'NA', object)
    if ok.any():
        out[ok] = abi.format_repr_f64(a[ok] / b[ok])
    return out


def write_pnps(args, tables, samples, res):
    blocks = [('_' + name, diversity.chain_cells(args, res['pi'][c], res['snps'][c], res['sites'][c], res['depth'][c]))
              for c, name in enumerate(CLASSES)]
    diversity.write_chains(args, tables, samples, blocks, extra=('pnps', ratio_cells(blocks[0][1], blocks[1][1])))


def run_pipeline(args, make_context=S.device_context):
    """diversity.run_pipeline for the two classes at once.  --seed: both global random streams are seeded before anything
    draws from them."""
    if args.get('seed') is not None:
        np.random.seed(args['seed'])
        random.seed(args['seed'])
    print("\nSelecting subset of samples...")
    tables = S.open_tables(args['indir'])
    samples = S.fetch_samples(tables, args['sample_depth'], args['fract_cov'], args['max_samples'], args['keep_samples'],
                              args['exclude_samples'], args['rand_samples'])
    print(" %s samples selected" % len(samples))
    print("Estimating pN/pS...\n")
    ctx = make_context()
    try:
        res = compute(args, tables, samples, ctx)
    finally:
        ctx.close()
    write_pnps(args, tables, samples, res)
    return res
