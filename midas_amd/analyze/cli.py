"""The command lines of snp_diversity.py, snp_pnps.py, snp_pairs.py, snp_trees.py, snp_ld.py, call_consensus.py, strain_tracking.py and compare_genes.py: the reference's option
names, defaults, check_args messages and printed argument block (scripts/snp_diversity.py:12-180, scripts/call_consensus.py:13-146,
scripts/strain_tracking.py:10-137, scripts/compare_genes.py:10-65), shared where they agree."""
import argparse
import os
import sys

INF = float('Inf')
MAX_RAND_READS = 2 ** 31 - 1

SAMPLE_OPTIONS = [
    (['--sample_depth'], dict(dest='sample_depth', type=float, default=0.0, metavar='FLOAT', help="samples with at least this mean_coverage (0.0)")),
    (['--sample_cov'], dict(dest='fract_cov', type=float, default=0.0, metavar='FLOAT',
                            help="samples with at least this fraction of the reference covered by a read (0.0)")),
    (['--max_samples'], dict(type=int, default=INF, metavar='INT', help="use at most this many samples, in snps_summary.txt order (all)")),
    (['--keep_samples'], dict(type=str, metavar='STR', help="comma-separated sample ids to use; the other sample filters still apply")),
    (['--exclude_samples'], dict(type=str, metavar='STR', help="comma-separated sample ids to leave out")),
]

SITE_OPTIONS = [
    (['--site_list'], dict(metavar='PATH', type=str, help="file with one site id per line: only these sites")),
    (['--site_depth'], dict(type=int, default=2, metavar='INT', help="a sample counts at a site with at least this many reads (2)")),
    (['--site_prev'], dict(type=float, default=0.0, metavar='FLOAT',
                           help="keep sites where at least this fraction of the samples counts (0.0: every site;\n1.0: sites covered in all samples)")),
    (['--site_maf'], dict(type=float, default=0.0, metavar='FLOAT',
                          help="keep sites whose pooled minor allele frequency is at least this (0.0: invariant sites too)")),
    (['--site_ratio'], dict(type=float, default=INF, metavar='FLOAT',
                            help="a sample counts at a site with at most this depth / mean_coverage (no limit)")),
    (['--allele_support'], dict(type=float, default=0.5, metavar='FLOAT',
                                help="a sample counts at a site when its commoner allele has at least this share of the reads (0.5)")),
    (['--locus_type'], dict(choices=['CDS', 'RNA', 'IGR'], help="only sites in coding genes (CDS), rRNA / tRNA genes (RNA) or between genes (IGR)")),
    (['--site_type'], dict(choices=['1D', '2D', '3D', '4D'], help="with --locus_type CDS: only sites of this degeneracy (4D synonymous, 1D not)")),
    (['--max_sites'], dict(type=int, default=INF, metavar='INT', help="stop after this many retained sites (all)")),
]

DIVERSITY_OPTIONS = [
    (['--genomic_type'], dict(choices=['genome-wide', 'per-gene'], default='genome-wide', help="one result for the genome, or one per gene (genome-wide)")),
    (['--sample_type'], dict(choices=['per-sample', 'pooled-samples'], default='per-sample',
                             help="one result per sample, or one for the samples pooled (per-sample)")),
    (['--weight_by_depth'], dict(action='store_true', default=False, help="pooled-samples: weight each sample by its depth at the site")),
    (['--rand_reads'], dict(type=int, metavar='INT',
                            help="rarefy: at every retained variable site give each sample N reads, round(freq x N) of them the minor\n"
                                 "allele, and compute from these; --site_depth is raised to N (numpy's global random stream)")),
    (['--replace_reads'], dict(action='store_true', default=False,
                               help="with --rand_reads: draw the N reads with replacement (without, the N reads are all of them)")),
    (['--rand_samples'], dict(type=int, metavar='INT', help="use a random subset of N samples (numpy's global random stream)")),
    (['--rand_sites'], dict(type=float, metavar='FLOAT', help="use a random share X of the sites (Python's global random stream)")),
    (['--snp_maf'], dict(type=float, metavar='FLOAT', default=0.01, help="a site is a SNP at or above this minor allele frequency (0.01)")),
    (['--consensus'], dict(action='store_true', default=False, help="round every frequency to 0 or 1 before anything is computed from it")),
]

SEED_OPTIONS = [
    (['--seed'], dict(type=int, metavar='INT', help="seed numpy's and Python's global random streams with INT first: --rand_samples,\n"
                                                    "--rand_sites and --rand_reads then give the same result every run")),
]

DEVICE_OPTIONS = [
    (['--group_rows'], dict(type=int, default=0, metavar='INT', help="matrix rows on the device at a time (0: what its memory holds);\nthe output does not depend on it")),
]


def _parser(prog, description, epilog, groups):
    parser = argparse.ArgumentParser(prog=prog, formatter_class=argparse.RawTextHelpFormatter, description=description, epilog=epilog)
    parser.add_argument('indir', metavar='PATH', type=str,
                        help="one species directory written by `merge_midas.py snps` (holds snps_freq.txt, snps_depth.txt,\nsnps_info.txt, snps_summary.txt)")
    parser.add_argument('--out', metavar='PATH', type=str, default='/dev/stdout', help="output file (/dev/stdout)")
    for title, options in groups:
        group = parser.add_argument_group(title)
        for flags, kw in options:
            group.add_argument(*flags, **kw)
    return parser


def diversity_arguments(argv=None):
    parser = _parser('snp_diversity.py',
                     "Nucleotide diversity (pi) and SNP density of one species from its merged SNP tables:\n"
                     "genome-wide or per gene, per sample or for the samples pooled.  Run `merge_midas.py snps` first.",
                     "examples:\n"
                     "  snp_diversity.py OUT/species_1 --genomic_type genome-wide --sample_type per-sample --out pi.txt\n"
                     "  snp_diversity.py OUT/species_1 --genomic_type per-gene --sample_type pooled-samples --locus_type CDS --out pi.txt\n"
                     "  snp_diversity.py OUT/species_1 --sample_type pooled-samples --locus_type CDS --site_type 4D --out pi.txt\n"
                     "  snp_diversity.py OUT/species_1 --max_sites 10000 --out pi.txt",
                     [("Diversity options", DIVERSITY_OPTIONS + SEED_OPTIONS), ("Sample filters", SAMPLE_OPTIONS), ("Site filters", SITE_OPTIONS),
                      ("Device", DEVICE_OPTIONS)])
    args = vars(parser.parse_args(argv))
    if args['rand_reads'] is not None and not 0 <= args['rand_reads'] <= MAX_RAND_READS:
        parser.error("--rand_reads must be between 0 and %d" % MAX_RAND_READS)
    if args['rand_reads']:          # (parse_arguments: a sample counts at a site only with N reads to pick from)
        args['site_depth'] = max(args['site_depth'], args['rand_reads'])
    return args


PNPS_LEFT_OUT = ('--rand_reads', '--replace_reads', '--locus_type', '--site_type')
PNPS_MAX_SITES_HELP = ("stop after this many retained sites, 1D and 4D sites counted together (all): a quick test.\n"
                       "Each of the two snp_diversity.py runs would stop at its own N-th site, so with this option the\n"
                       "blocks are not theirs")


def pnps_arguments(argv=None):
    """snp_pnps.py: snp_diversity.py's options under their names and defaults, without --locus_type / --site_type (the classes
    are CDS 1D and CDS 4D) and without --rand_reads / --replace_reads."""
    helps = {'--max_sites': PNPS_MAX_SITES_HELP,
             '--seed': "seed numpy's and Python's global random streams with INT first: --rand_samples and\n--rand_sites then give the same result every run"}
    keep = lambda options: [(f, dict(kw, help=helps[f[0]]) if f[0] in helps else kw) for f, kw in options if f[0] not in PNPS_LEFT_OUT]
    parser = _parser('snp_pnps.py',
                     "pN/pS of one species from its merged SNP tables: nucleotide diversity and SNP density at the\n"
                     "non-degenerate (1D) and at the four-fold degenerate (4D) sites of coding genes, and the ratio of the two\n"
                     "pi_bp -- genome-wide or per gene, per sample or for the samples pooled.  Each block of columns is what\n"
                     "`snp_diversity.py --locus_type CDS --site_type 1D` (or 4D) writes; both come from one pass over the matrices.\n"
                     "--rand_reads / --replace_reads are not offered: the two separate runs draw the random stream over\n"
                     "different sets of sites, so no single pass gives what both give.  Run `merge_midas.py snps` first.",
                     "examples:\n"
                     "  snp_pnps.py OUT/species_1 --sample_type pooled-samples --genomic_type per-gene --out pnps.txt\n"
                     "  snp_pnps.py OUT/species_1 --site_prev 0.9 --site_depth 5 --out pnps.txt\n\n"
                     "output: per chain depth (per-sample), sites, snps, pi, snps_kb, pi_bp with the suffix _1D, the same with _4D,\n"
                     "and pnps = pi_bp_1D / pi_bp_4D (NA where either is NA or pi_bp_4D is 0.0)",
                     [("pN/pS options", keep(DIVERSITY_OPTIONS + SEED_OPTIONS)), ("Sample filters", SAMPLE_OPTIONS), ("Site filters", keep(SITE_OPTIONS)),
                      ("Device", DEVICE_OPTIONS)])
    return vars(parser.parse_args(argv))


PAIRS_LEFT_OUT = ('--genomic_type', '--sample_type', '--rand_reads', '--replace_reads')
PAIRS_OPTIONS = [
    (['--tree'], dict(metavar='PATH', type=str, help="also write a neighbour-joining tree over da (dxy minus the mean within-sample pi_bp)\nhere, in Newick format; needs at least 3 samples")),
]
PAIRS_DEVICE_OPTIONS = DEVICE_OPTIONS + [(['--chunk_bytes'], dict(type=int, default=0, help=argparse.SUPPRESS)),
                                         (['--pair_form'], dict(type=int, default=0, choices=[0, 1, 2], help=argparse.SUPPRESS))]


def pairs_arguments(argv=None):
    """snp_pairs.py: snp_diversity.py's sample, site and diversity options under their names and defaults, without --genomic_type /
    --sample_type (always genome-wide over pooled pairs) and without --rand_reads / --replace_reads; --tree; the hidden
    --chunk_bytes and --pair_form."""
    helps = {'--max_sites': "every pair stops after this many retained sites of its own (all)",
             '--weight_by_depth': "weight each of the two samples by its depth at the site",
             '--seed': "seed numpy's and Python's global random streams with INT first: --rand_samples and\n--rand_sites then give the same result every run"}
    keep = lambda options: [(f, dict(kw, help=helps[f[0]]) if f[0] in helps else kw) for f, kw in options if f[0] not in PAIRS_LEFT_OUT]
    parser = _parser('snp_pairs.py',
                     "Between-sample heterogeneity of one species for every pair of samples, from its merged SNP tables: what\n"
                     "`snp_diversity.py --sample_type pooled-samples --keep_samples a,b` writes for the pair (a, b), and beside it,\n"
                     "over the sites both samples are kept at, the pi_bp within each sample, the pi_bp between them (dxy),\n"
                     "Hudson's Fst and da.  All pairs come from one pass over the matrices.  Run `merge_midas.py snps` first.\n"
                     "--genomic_type / --sample_type are not offered: the command is always genome-wide over pooled pairs.\n"
                     "--rand_reads / --replace_reads are not offered: each separate run draws the random stream from its own\n"
                     "start over its own sites, so no single pass gives what they give.",
                     "examples:\n"
                     "  snp_pairs.py OUT/species_1 --out pairs.txt\n"
                     "  snp_pairs.py OUT/species_1 --out pairs.txt --tree da.nwk --site_depth 5 --site_prev 1.0 --sample_depth 10\n\n"
                     "output: sample1, sample2, then samples (2), sites, snps, pi, snps_kb, pi_bp of the pooled pair, then shared_sites,\n"
                     "pi_bp_1, pi_bp_2, dxy, fst = 1 - ((pi_bp_1 + pi_bp_2) / 2) / dxy and da = dxy - (pi_bp_1 + pi_bp_2) / 2\n"
                     "(NA without a shared site; fst also where dxy is 0.0)",
                     [("Pair options", PAIRS_OPTIONS + keep(DIVERSITY_OPTIONS + SEED_OPTIONS)), ("Sample filters", SAMPLE_OPTIONS),
                      ("Site filters", keep(SITE_OPTIONS)), ("Device", PAIRS_DEVICE_OPTIONS)])
    return vars(parser.parse_args(argv))


def consensus_arguments(argv=None):
    parser = _parser('call_consensus.py',
                     "One consensus sequence per sample over the retained sites of a species, as a multi-FASTA (for trees).\n"
                     "Run `merge_midas.py snps` first.",
                     "examples:\n"
                     "  call_consensus.py OUT/species_1 --out seqs.fa --site_maf 0.01 --site_depth 5 --site_prev 0.90 \\\n"
                     "      --sample_depth 10 --sample_cov 0.40 --site_ratio 5.0\n"
                     "  call_consensus.py OUT/species_1 --out seqs.fa --max_sites 10000",
                     [("Sample filters", SAMPLE_OPTIONS), ("Site filters", SITE_OPTIONS), ("Device", DEVICE_OPTIONS)])
    return vars(parser.parse_args(argv))


def print_args(args, script):
    """The reference's argument block, line for line (its last but one line prints locus_type under the name site_type).
    snp_pnps.py and snp_pairs.py are not the reference's: the same block with the options they have (snp_pairs.py prints
    site_type under its own name)."""
    rows = [("Command: %s" % ' '.join(sys.argv)), "Script: %s" % script, "Input directory: %s" % args['indir'], "Output file: %s" % args['out']]
    blocks = []
    if script == 'snp_diversity.py':
        blocks.append(("Diversity options:", ['genomic_type', 'sample_type', 'weight_by_depth', 'rand_reads', 'replace_reads', 'rand_samples',
                                              'rand_sites', 'snp_maf', 'consensus']))
    if script == 'snp_pnps.py':
        blocks.append(("pN/pS options:", ['genomic_type', 'sample_type', 'weight_by_depth', 'rand_samples', 'rand_sites', 'snp_maf', 'consensus']))
    if script == 'snp_pairs.py':
        blocks.append(("Pair options:", ['tree', 'weight_by_depth', 'rand_samples', 'rand_sites', 'snp_maf', 'consensus']))
    blocks.append(("Sample filters:", ['sample_depth', 'fract_cov', 'max_samples', 'keep_samples', 'exclude_samples']))
    blocks.append(("Site filters:", ['site_list', 'site_depth', 'site_prev', 'site_maf', 'site_ratio', 'allele_support', 'locus_type', 'site_type',
                                     'max_sites']))
    for title, names in blocks:
        rows.append(title)
        for name in names:
            if script == 'snp_pnps.py' and name in ('locus_type', 'site_type'):
                continue
            rows.append("  %s: %s" % (name, args['locus_type' if name == 'site_type' and script != 'snp_pairs.py' else name]))
    sys.stdout.write('\n'.join(rows) + '\n')


def _exit(message):
    sys.exit("\nError: %s\n" % message)


def _common_checks(args):
    if args['max_sites'] < 1:
        _exit("--max_sites must be >= 1 to calculate nucleotide variation")
    if args['max_samples'] < 1:
        _exit("--max_samples must be >= 1 to calculate nucleotide variation")
    if args['site_ratio'] < 0:
        _exit("--site_ratio cannot be a negative number")
    if args['site_depth'] < 0:
        _exit("--site_depth cannot be a negative number")
    if args['sample_depth'] < 0:
        _exit("--sample_depth cannot be a negative number")
    if not 0 <= args['site_maf'] <= 1:
        _exit("--site_maf must be between 0 and 1")
    if not 0 <= args['site_prev'] <= 1:
        _exit("--site_prev must be between 0 and 1")
    if not 0 <= args['fract_cov'] <= 1:
        _exit("--fract_cov must be between 0 and 1")


def check_diversity_args(args, resampling=False):
    """check_args of snp_diversity.py, in its order.  Its --rand_reads comparison cannot run under Python 3 without the
    option, and with it never fires: diversity_arguments has raised --site_depth to --rand_reads.  It keeps its place.
    resampling: what follows runs --rand_reads / --replace_reads (diversity.run_pipeline does; the command passes True).  A
    caller that does not say so gets the answer these options had before the device could resample: the exit below."""
    if not resampling and (args['rand_reads'] is not None or args['replace_reads']):
        _exit("--rand_reads / --replace_reads are not part of this build")
    if not os.path.isdir(args['indir']):
        _exit("Specified input directory '%s' does not exist" % args['indir'])
    if args['site_depth'] < 2:
        _exit("--site_depth must be >=2 to calculate nucleotide variation")
    _common_checks(args)
    if args['rand_reads'] and args['rand_reads'] > args['site_depth'] and not args['replace_reads']:
        _exit("--rand_reads cannot exceed --site_depth when --replace_reads=False")
    if args['rand_sites'] and (args['rand_sites'] < 0 or args['rand_sites'] > 1):
        _exit("--rand_sites must be between 0 and 1")
    if args['locus_type'] != 'CDS' and args['genomic_type'] == 'per-gene':
        _exit("--locus_type must be CDS if --genomic_type is per-gene")
    if args['locus_type'] != 'CDS' and args['site_type'] is not None:
        _exit("--locus_type must be CDS if --site_type is specified")


def check_pnps_args(args):
    """check_diversity_args' checks that still apply: the classes are CDS sites, and nothing is resampled."""
    if not os.path.isdir(args['indir']):
        _exit("Specified input directory '%s' does not exist" % args['indir'])
    if args['site_depth'] < 2:
        _exit("--site_depth must be >=2 to calculate nucleotide variation")
    _common_checks(args)
    if args['rand_sites'] and (args['rand_sites'] < 0 or args['rand_sites'] > 1):
        _exit("--rand_sites must be between 0 and 1")


def check_pairs_args(args):
    """check_diversity_args' checks that still apply: nothing is resampled and nothing is per gene."""
    check_pnps_args(args)
    if args['locus_type'] != 'CDS' and args['site_type'] is not None:
        _exit("--locus_type must be CDS if --site_type is specified")


def check_consensus_args(args):
    if not os.path.isdir(args['indir']):
        _exit("Specified input directory '%s' does not exist" % args['indir'])
    if args['site_depth'] < 1:
        _exit("--site_depth must be >=1")
    _common_checks(args)


TREE_OPTIONS = [
    (['--dist'], dict(metavar='PATH', type=str, help="also write the table of pairwise distances here:\nsample1, sample2, sites, mismatches, distance")),
]
HIDDEN_DEVICE_OPTIONS = [(['--group_rows'], dict(type=int, default=0, help=argparse.SUPPRESS))]
NEWICK_SPECIAL = "()[]':;,"


def trees_arguments(argv=None):
    """snp_trees.py: the sample and site options of call_consensus.py under their names and defaults, --dist, the hidden
    --group_rows.  --out is the Newick file."""
    parser = _parser('snp_trees.py',
                     "A core-genome tree of the samples of one species: the consensus allele of every sample at the retained\n"
                     "sites (as call_consensus.py calls it), the share of differing sites between every two samples, and a\n"
                     "neighbour-joining tree over these distances, in Newick format.  Run `merge_midas.py snps` first.",
                     "examples:\n"
                     "  snp_trees.py OUT/species_1 --out tree.nwk --dist pairs.txt --site_maf 0.01 --site_depth 5 --site_prev 0.90 \\\n"
                     "      --sample_depth 10 --sample_cov 0.40 --site_ratio 5.0\n"
                     "  snp_trees.py OUT/species_1 --out tree.nwk --exclude_samples s7,s9 --max_sites 10000",
                     [("Tree options", TREE_OPTIONS), ("Sample filters", SAMPLE_OPTIONS), ("Site filters", SITE_OPTIONS),
                      ("Device", HIDDEN_DEVICE_OPTIONS)])
    return vars(parser.parse_args(argv))


def check_trees_args(args):
    if not os.path.isdir(args['indir']):
        _exit("Specified input directory '%s' does not exist" % args['indir'])
    if args['site_depth'] < 1:
        _exit("--site_depth must be >=1")
    _common_checks(args)


def check_tree_samples(sample_ids):
    """A tree has at least three leaves, and a leaf is written as it is: no Newick quoting."""
    if len(sample_ids) < 3:
        _exit("a tree needs at least 3 samples; %d selected" % len(sample_ids))
    for sample_id in sample_ids:
        if any(c.isspace() or c in NEWICK_SPECIAL for c in sample_id):
            _exit("the sample id '%s' contains whitespace or one of %s, which a Newick label cannot hold" % (sample_id, NEWICK_SPECIAL))


def print_trees_args(args):
    rows = ["Command: %s" % ' '.join(sys.argv), "Script: snp_trees.py", "Input directory: %s" % args['indir'], "Output file: %s" % args['out'],
            "Distance table: %s" % args['dist']]
    for title, names in (("Sample filters:", ['sample_depth', 'fract_cov', 'max_samples', 'keep_samples', 'exclude_samples']),
                         ("Site filters:", ['site_list', 'site_depth', 'site_prev', 'site_maf', 'site_ratio', 'allele_support', 'locus_type',
                                            'site_type', 'max_sites'])):
        rows.append(title)
        rows.extend("  %s: %s" % (name, args[name]) for name in names)
    sys.stdout.write('\n'.join(rows) + '\n')


LD_MAX_BINS = 4096          # abi.SITES_LD_MAX_BINS
LD_MAX_DIST = 2 ** 39       # the site keys keep 2^40 positions a contig
LD_OPTIONS = [
    (['--max_dist'], dict(type=int, default=1000, metavar='INT', help="the largest distance in bases between the two sites of a pair (1000)")),
    (['--bin_width'], dict(type=int, default=10, metavar='INT',
                           help="bases a distance bin: bin k holds the distances k x B + 1 ... (k + 1) x B (10); at most %d bins" % LD_MAX_BINS)),
    (['--min_samples'], dict(type=int, default=4, metavar='INT', help="a pair of sites counts only with this many samples called at both (4)")),
    (['--within'], dict(choices=['contig', 'gene'], default='contig',
                        help="pair two sites of one contig, or only two sites of one gene (contig)")),
]
LD_DEVICE_OPTIONS = HIDDEN_DEVICE_OPTIONS + [(['--chunk_bytes'], dict(type=int, default=0, help=argparse.SUPPRESS)),
                                             (['--anchor_chunk'], dict(type=int, default=0, help=argparse.SUPPRESS))]


def ld_arguments(argv=None):
    """snp_ld.py: the sample and site options of snp_trees.py under their names and defaults, the four options of its own, the
    hidden --group_rows, --chunk_bytes and --anchor_chunk."""
    parser = _parser('snp_ld.py',
                     "Linkage disequilibrium between the sites of one species, by distance: the consensus allele of every sample\n"
                     "at the retained sites (as call_consensus.py calls it), and for every pair of sites at most --max_dist bases\n"
                     "apart r2 and the terms of sigma2_d over the samples called at both, averaged per distance bin.  LD that\n"
                     "decays with distance tells a recombining population from a clonal one.  Run `merge_midas.py snps` first.",
                     "examples:\n"
                     "  snp_ld.py OUT/species_1 --out ld.txt --site_depth 5 --site_prev 0.90 --sample_depth 10\n"
                     "  snp_ld.py OUT/species_1 --out ld.txt --max_dist 3000 --bin_width 50 --within gene --locus_type CDS\n\n"
                     "output: bin_start, bin_end (distances in bases), site_pairs (pairs of retained sites in the bin), ld_pairs (those\n"
                     "with --min_samples samples called at both sites and both alleles seen at each), r2 = their mean r2, and\n"
                     "sigma2_d = sum of D2 / sum of the heterozygosity products (NA without an ld_pair)",
                     [("LD options", LD_OPTIONS), ("Sample filters", SAMPLE_OPTIONS), ("Site filters", SITE_OPTIONS), ("Device", LD_DEVICE_OPTIONS)])
    return vars(parser.parse_args(argv))


def check_ld_args(args):
    check_trees_args(args)
    if args['max_dist'] < 1:
        _exit("--max_dist must be >= 1")
    if args['max_dist'] >= LD_MAX_DIST:
        _exit("--max_dist must be below 2^39")
    if args['bin_width'] < 1:
        _exit("--bin_width must be >= 1")
    if -(-args['max_dist'] // args['bin_width']) > LD_MAX_BINS:
        _exit("--max_dist / --bin_width gives more than %d distance bins: raise --bin_width" % LD_MAX_BINS)
    if args['min_samples'] < 1:
        _exit("--min_samples must be >= 1")
    if args['group_rows'] < 0 or args['chunk_bytes'] < 0 or args['anchor_chunk'] < 0:
        _exit("--group_rows, --chunk_bytes and --anchor_chunk cannot be negative")


def print_ld_args(args):
    rows = ["Command: %s" % ' '.join(sys.argv), "Script: snp_ld.py", "Input directory: %s" % args['indir'], "Output file: %s" % args['out']]
    for title, names in (("LD options:", ['max_dist', 'bin_width', 'min_samples', 'within']),
                         ("Sample filters:", ['sample_depth', 'fract_cov', 'max_samples', 'keep_samples', 'exclude_samples']),
                         ("Site filters:", ['site_list', 'site_depth', 'site_prev', 'site_maf', 'site_ratio', 'allele_support', 'locus_type',
                                            'site_type', 'max_sites'])):
        rows.append(title)
        rows.extend("  %s: %s" % (name, args[name]) for name in names)
    sys.stdout.write('\n'.join(rows) + '\n')


STRAIN_COMMANDS = ['id_markers', 'track_markers']
STRAIN_USAGE = ['', 'Usage: strain_tracking.py <command> [options]', '',
                'Note: use strain_tracking.py <command> -h to view usage for a specific command', '', 'Commands:',
                '\tid_markers      identify rare SNPs that disriminate individual strains',
                '\ttrack_markers   track rare SNPs between samples and determine transmission']

CALL_OPTIONS = [
    (['--min_freq'], dict(type=float, metavar='FLOAT', default=0.10, help="an allele counts in a sample from this share of the reads at the site (0.10)")),
    (['--min_reads'], dict(type=int, metavar='INT', default=3, help="... and from this many reads, round(share x depth) (3)")),
]


def strain_program(argv=None):
    """get_program: the usage screen without a command or with -h, the exit for a command that is not one."""
    argv = sys.argv[1:] if argv is None else argv
    if len(argv) == 0 or argv[0] in ['-h', '--help']:
        sys.stdout.write('\n'.join(STRAIN_USAGE) + '\n')
        sys.exit()
    if argv[0] not in STRAIN_COMMANDS:
        _exit("Unrecognized command: '%s'" % argv[0])
    return argv[0]


def _strain_parser(command, description, epilog, options):
    parser = argparse.ArgumentParser(prog='strain_tracking.py %s' % command, formatter_class=argparse.RawTextHelpFormatter,
                                     usage=argparse.SUPPRESS,
                                     description="\nDescription: %s\n\nUsage: strain_tracking.py %s [options]\n" % (description, command), epilog=epilog)
    parser.add_argument('program', help=argparse.SUPPRESS)
    parser.add_argument('--indir', metavar='PATH', type=str, required=True,
                        help="one species directory written by `merge_midas.py snps` (holds snps_freq.txt, snps_depth.txt,\nsnps_info.txt, snps_summary.txt)")
    for flags, kw in options + DEVICE_OPTIONS:
        parser.add_argument(*flags, **kw)
    return parser


def id_markers_arguments(argv=None):
    """id_arguments: argv starts with the command.  --samples becomes a list: membership in it is list membership."""
    parser = _strain_parser('id_markers', "find the rare alleles that tell the strains of one species apart",
                            "examples:\n"
                            "  strain_tracking.py id_markers --indir OUT/species_1 --out markers.txt --samples s1,s2,s3\n"
                            "  strain_tracking.py id_markers --indir OUT/species_1 --out markers.txt --max_sites 10000\n\n"
                            "output: site_id, allele, count_samples (samples with a read at the site) and count_A, count_T, count_C,\n"
                            "count_G (samples that have the letter) per marker",
                            [(['--out'], dict(metavar='PATH', type=str, required=True, help="output file: the list of markers")),
                             (['--samples'], dict(metavar='STR', type=str, help="comma-separated training samples (all)"))] + CALL_OPTIONS +
                            [(['--allele_prev'], dict(type=int, metavar='INT', default=1,
                                                      help="a marker allele is found in at most this many samples (1: in exactly one)")),
                             (['--max_sites'], dict(type=int, metavar='INT', default=INF, help="stop after this many sites read (all)"))])
    args = vars(parser.parse_args(argv))
    if args['samples']:
        args['samples'] = args['samples'].split(',')
    return args


def track_markers_arguments(argv=None):
    """track_arguments with its two existence checks; --out or --markers left out is a plain error here."""
    parser = _strain_parser('track_markers', "count the marker alleles every pair of samples shares",
                            "examples:\n"
                            "  strain_tracking.py track_markers --indir OUT/species_1 --markers markers.txt --out allele_sharing.txt\n"
                            "  strain_tracking.py track_markers --indir OUT/species_1 --markers markers.txt --out allele_sharing.txt --max_sites 1000\n\n"
                            "output: sample1, sample2, count1, count2 (marker alleles in each), count_both, count_either per pair",
                            [(['--out'], dict(metavar='PATH', type=str, help="output file: marker sharing of every pair of samples")),
                             (['--markers'], dict(metavar='PATH', type=str, help="the list `strain_tracking.py id_markers` wrote"))] + CALL_OPTIONS +
                            [(['--max_sites'], dict(type=int, metavar='INT', default=INF, help="stop after this many sites read (all)")),
                             (['--max_samples'], dict(type=int, metavar='INT', help="(accepted; as in the reference it is never applied)"))])
    args = vars(parser.parse_args(argv))
    if not os.path.isdir(args['indir']):
        _exit("Specified input directory '%s' does not exist" % args['indir'])
    if args['markers'] is None:
        _exit("--markers is required")
    if not os.path.isfile(args['markers']):
        _exit("Specified input file '%s' does not exist" % args['markers'])
    if args['out'] is None:
        _exit("--out is required")
    return args


def compare_genes_arguments(argv=None):
    """parse_arguments + init_paths of compare_genes.py: its screen layout (no usage line of argparse's own), option names and
    defaults; the three genes_*.txt must exist, though only the copy numbers are read.  --group_rows is hidden."""
    parser = argparse.ArgumentParser(
        prog='compare_genes.py', formatter_class=argparse.RawTextHelpFormatter, usage=argparse.SUPPRESS,
        description="Description:\nDistances between the gene content of all pairs of samples of one species, on the device.\n"
                    "Run `merge_midas.py genes` first.\n\nUsage: compare_genes.py indir [options]\n",
        epilog="Examples:\n"
               "1) defaults (presence / absence at copy number 0.35, Jaccard distance):\n"
               "compare_genes.py OUT/species_1 --out distances.txt\n\n"
               "2) a quick look at part of the matrix:\n"
               "compare_genes.py OUT/species_1 --out distances.txt --max_genes 1000 --max_samples 10\n\n"
               "3) another metric, on the copy numbers themselves:\n"
               "compare_genes.py OUT/species_1 --out distances.txt --dtype copynum --distance manhattan\n\n"
               "4) a lenient or a strict call of presence:\n"
               "compare_genes.py OUT/species_1 --out distances.txt --cutoff 0.10\n"
               "compare_genes.py OUT/species_1 --out distances.txt --cutoff 0.75\n")
    parser.add_argument('indir', metavar='PATH', type=str,
                        help="one species directory written by `merge_midas.py genes` (holds genes_presabs.txt,\n"
                             "genes_copynum.txt, genes_depth.txt)")
    parser.add_argument('--out', metavar='PATH', type=str, default='/dev/stdout', help="output file (/dev/stdout)")
    parser.add_argument('--max_genes', metavar='INT', type=int, help="read this many genes (rows) only (all)")
    parser.add_argument('--max_samples', metavar='INT', type=int, help="use the first INT samples (columns) only (all)")
    parser.add_argument('--distance', choices=['jaccard', 'euclidean', 'manhattan'], default='jaccard', help="the distance (jaccard)")
    parser.add_argument('--dtype', choices=['presabs', 'copynum'], default='presabs',
                        help="compare presence / absence or the copy numbers (presabs)")
    parser.add_argument('--cutoff', metavar='FLOAT', type=float, default=0.35,
                        help="presabs: a gene is present above this copy number (0.35)")
    parser.add_argument('--group_rows', type=int, default=0, help=argparse.SUPPRESS)
    args = vars(parser.parse_args(argv))
    for ext in ['presabs', 'depth', 'copynum']:
        inpath = '%s/genes_%s.txt' % (args['indir'], ext)
        if not os.path.isfile(inpath):
            sys.exit("\nError: Input file does not exist: %s\n" % inpath)
        args[ext] = inpath
    return args


def gene_linkage_arguments(argv=None):
    """gene_linkage.py: the screen layout and the input rules of compare_genes.py; the linkage options are checked here, each
    broken rule ends with the Error exit.  --group_rows and --chunk_bytes are hidden."""
    parser = argparse.ArgumentParser(
        prog='gene_linkage.py', formatter_class=argparse.RawTextHelpFormatter, usage=argparse.SUPPRESS,
        description="Description:\nPairs of genes of one species that are present in the same samples, and the groups those pairs form,\n"
                    "on the device.  Run `merge_midas.py genes` first.\n\nUsage: gene_linkage.py indir [options]\n",
        epilog="Examples:\n"
               "1) defaults (presence above copy number 0.35, pairs at a Jaccard index of 0.9 and above):\n"
               "gene_linkage.py OUT/species_1 --out pairs.txt --groups groups.txt\n\n"
               "2) identical profiles only, among genes found in at least 5 samples and missing from at least 5:\n"
               "gene_linkage.py OUT/species_1 --out pairs.txt --min_jaccard 1.0 --min_present 5 --min_absent 5\n\n"
               "3) looser links, groups of three genes and more:\n"
               "gene_linkage.py OUT/species_1 --out pairs.txt --groups groups.txt --min_jaccard 0.75 --min_group 3\n")
    parser.add_argument('indir', metavar='PATH', type=str,
                        help="one species directory written by `merge_midas.py genes` (holds genes_presabs.txt,\n"
                             "genes_copynum.txt, genes_depth.txt)")
    parser.add_argument('--out', metavar='PATH', type=str, default='/dev/stdout', help="the table of linked pairs (/dev/stdout)")
    parser.add_argument('--groups', metavar='PATH', type=str, help="the table of linkage groups (not written)")
    parser.add_argument('--max_genes', metavar='INT', type=int, help="read this many genes (rows) only (all)")
    parser.add_argument('--max_samples', metavar='INT', type=int, help="use the first INT samples (columns) only (all)")
    parser.add_argument('--cutoff', metavar='FLOAT', type=float, default=0.35, help="a gene is present above this copy number (0.35)")
    parser.add_argument('--min_present', metavar='INT', type=int, default=2, help="keep genes present in at least INT samples (2)")
    parser.add_argument('--min_absent', metavar='INT', type=int, default=2, help="keep genes absent from at least INT samples (2)")
    parser.add_argument('--min_jaccard', metavar='FLOAT', type=float, default=0.9,
                        help="link two genes when samples with both / samples with either >= FLOAT (0.9)")
    parser.add_argument('--min_group', metavar='INT', type=int, default=2, help="write groups of at least INT genes (2)")
    parser.add_argument('--max_pairs', metavar='INT', type=int, default=1 << 26, help="stop when more pairs than this are linked (67108864)")
    parser.add_argument('--group_rows', type=int, default=0, help=argparse.SUPPRESS)
    parser.add_argument('--chunk_bytes', type=int, default=0, help=argparse.SUPPRESS)
    args = vars(parser.parse_args(argv))
    for ext in ['presabs', 'depth', 'copynum']:
        inpath = '%s/genes_%s.txt' % (args['indir'], ext)
        if not os.path.isfile(inpath):
            sys.exit("\nError: Input file does not exist: %s\n" % inpath)
        args[ext] = inpath
    if args['cutoff'] != args['cutoff'] or args['cutoff'] in (float('inf'), float('-inf')):
        _exit("--cutoff must be a finite number")
    if args['min_present'] < 1:
        _exit("--min_present must be >= 1: a gene found in no sample has no partner")
    if args['min_absent'] < 0:
        _exit("--min_absent cannot be a negative number")
    if not 0 < args['min_jaccard'] <= 1:
        _exit("--min_jaccard must be above 0 and at most 1")
    if args['min_group'] < 2:
        _exit("--min_group must be >= 2: a group is two linked genes or more")
    if not 0 <= args['max_pairs'] < 1 << 31:
        _exit("--max_pairs must be between 0 and 2147483647")
    if args['group_rows'] < 0:
        _exit("--group_rows cannot be a negative number")
    if args['chunk_bytes'] < 0:
        _exit("--chunk_bytes cannot be a negative number")
    return args


def gene_assoc_arguments(argv=None):
    """gene_assoc.py: the screen layout and the input rules of compare_genes.py; the test's options are checked here, each broken
    rule ends with the Error exit (the rules of the --groups file are genes_assoc.read_groups').  --group_rows, --chunk_bytes and
    --form are hidden."""
    parser = argparse.ArgumentParser(
        prog='gene_assoc.py', formatter_class=argparse.RawTextHelpFormatter, usage=argparse.SUPPRESS,
        description="Description:\nGenes of one species whose presence or copy number differs between two groups of samples, with a\n"
                    "permutation test, on the device.  Run `merge_midas.py genes` first.\n\nUsage: gene_assoc.py indir --groups FILE [options]\n",
        epilog="Examples:\n"
               "1) presence / absence at copy number 0.35, Fisher's exact test:\n"
               "gene_assoc.py OUT/species_1 --groups groups.txt --out assoc.txt\n\n"
               "2) the same with 10 000 relabellings of the samples:\n"
               "gene_assoc.py OUT/species_1 --groups groups.txt --out assoc.txt --permutations 10000 --seed 7\n\n"
               "3) the copy numbers themselves (rank-sum test), genes found in at least 5 samples:\n"
               "gene_assoc.py OUT/species_1 --groups groups.txt --out assoc.txt --dtype copynum --min_present 5 --permutations 10000\n")
    parser.add_argument('indir', metavar='PATH', type=str,
                        help="one species directory written by `merge_midas.py genes` (holds genes_presabs.txt,\n"
                             "genes_copynum.txt, genes_depth.txt)")
    parser.add_argument('--groups', metavar='PATH', type=str, help="lines of sample_id<TAB>label with two distinct labels (required)")
    parser.add_argument('--case', metavar='LABEL', type=str, help="the label of the case group (the greater label in byte order)")
    parser.add_argument('--out', metavar='PATH', type=str, default='/dev/stdout', help="the table of genes (/dev/stdout)")
    parser.add_argument('--max_genes', metavar='INT', type=int, help="read this many genes (rows) only (all)")
    parser.add_argument('--max_samples', metavar='INT', type=int, help="use the first INT samples (columns) only (all)")
    parser.add_argument('--dtype', choices=['presabs', 'copynum'], default='presabs',
                        help="test presence / absence (Fisher's exact test) or the copy numbers (rank-sum test) (presabs)")
    parser.add_argument('--cutoff', metavar='FLOAT', type=float, default=0.35, help="a gene is present above this copy number (0.35)")
    parser.add_argument('--min_present', metavar='INT', type=int, default=1, help="keep genes present in at least INT used samples (1)")
    parser.add_argument('--min_absent', metavar='INT', type=int, default=0, help="keep genes absent from at least INT used samples (0)")
    parser.add_argument('--permutations', metavar='INT', type=int, default=0, help="relabellings of the samples for p_perm (0: none)")
    parser.add_argument('--seed', metavar='INT', type=int, default=0, help="seed of the relabellings (0)")
    parser.add_argument('--group_rows', type=int, default=0, help=argparse.SUPPRESS)
    parser.add_argument('--chunk_bytes', type=int, default=0, help=argparse.SUPPRESS)
    parser.add_argument('--form', type=int, default=1, help=argparse.SUPPRESS)
    args = vars(parser.parse_args(argv))
    for ext in ['presabs', 'depth', 'copynum']:
        inpath = '%s/genes_%s.txt' % (args['indir'], ext)
        if not os.path.isfile(inpath):
            sys.exit("\nError: Input file does not exist: %s\n" % inpath)
        args[ext] = inpath
    if args['groups'] is None:
        _exit("--groups is required")
    if not os.path.isfile(args['groups']):
        _exit("Specified input file '%s' does not exist" % args['groups'])
    if args['cutoff'] != args['cutoff'] or args['cutoff'] in (float('inf'), float('-inf')):
        _exit("--cutoff must be a finite number")
    if args['min_present'] < 0:
        _exit("--min_present cannot be a negative number")
    if args['min_absent'] < 0:
        _exit("--min_absent cannot be a negative number")
    if not 0 <= args['permutations'] <= 1000000:
        _exit("--permutations must be between 0 and 1000000")
    if args['seed'] < 0:
        _exit("--seed cannot be a negative number")
    if args['group_rows'] < 0:
        _exit("--group_rows cannot be a negative number")
    if args['chunk_bytes'] < 0:
        _exit("--chunk_bytes cannot be a negative number")
    if args['form'] not in (0, 1):
        _exit("--form must be 0 or 1")
    return args


def gene_curves_arguments(argv=None):
    """gene_curves.py: the screen layout and the input rules of compare_genes.py; the curves' options are checked here, each broken
    rule ends with the Error exit (the rules of the --samples file are genes_curves.read_samples').  --group_rows, --chunk_bytes
    and --form are hidden."""
    parser = argparse.ArgumentParser(
        prog='gene_curves.py', formatter_class=argparse.RawTextHelpFormatter, usage=argparse.SUPPRESS,
        description="Description:\nHow the pangenome of one species grows and its core genome shrinks as samples are added: accumulation\n"
                    "curves over the listed and over random orders of the samples, with Heaps' law, on the device.\n"
                    "Run `merge_midas.py genes` first.\n\nUsage: gene_curves.py indir [options]\n",
        epilog="Examples:\n"
               "1) defaults (presence above copy number 0.35, a core gene is in every sample, 100 random orders):\n"
               "gene_curves.py OUT/species_1 --out curves.txt\n\n"
               "2) a soft core (95 % of the samples so far), 1 000 orders, every order's curve kept:\n"
               "gene_curves.py OUT/species_1 --out curves.txt --core_frac 0.95 --permutations 1000 --seed 7 --orders orders.txt\n\n"
               "3) the listed order alone, over the samples a file names:\n"
               "gene_curves.py OUT/species_1 --out curves.txt --samples ids.txt --permutations 0\n")
    parser.add_argument('indir', metavar='PATH', type=str,
                        help="one species directory written by `merge_midas.py genes` (holds genes_presabs.txt,\n"
                             "genes_copynum.txt, genes_depth.txt)")
    parser.add_argument('--out', metavar='PATH', type=str, default='/dev/stdout', help="the table of curves, one row a number of samples (/dev/stdout)")
    parser.add_argument('--orders', metavar='PATH', type=str, help="the curve of every order, one row an order and sample (not written)")
    parser.add_argument('--samples', metavar='PATH', type=str, help="use the samples this file lists, one id a line (all)")
    parser.add_argument('--max_genes', metavar='INT', type=int, help="read this many genes (rows) only (all)")
    parser.add_argument('--max_samples', metavar='INT', type=int, help="use the first INT samples (columns) only (all)")
    parser.add_argument('--cutoff', metavar='FLOAT', type=float, default=0.35, help="a gene is present above this copy number (0.35)")
    parser.add_argument('--core_frac', metavar='FLOAT', type=float, default=1.0,
                        help="a gene is core while it is present in at least this share of the samples so far (1.0)")
    parser.add_argument('--permutations', metavar='INT', type=int, default=100, help="random orders of the samples beside the listed one (100)")
    parser.add_argument('--seed', metavar='INT', type=int, default=0, help="seed of the random orders (0)")
    parser.add_argument('--group_rows', type=int, default=0, help=argparse.SUPPRESS)
    parser.add_argument('--chunk_bytes', type=int, default=0, help=argparse.SUPPRESS)
    parser.add_argument('--form', type=int, default=1, help=argparse.SUPPRESS)
    args = vars(parser.parse_args(argv))
    for ext in ['presabs', 'depth', 'copynum']:
        inpath = '%s/genes_%s.txt' % (args['indir'], ext)
        if not os.path.isfile(inpath):
            sys.exit("\nError: Input file does not exist: %s\n" % inpath)
        args[ext] = inpath
    if args['samples'] is not None and not os.path.isfile(args['samples']):
        _exit("Specified input file '%s' does not exist" % args['samples'])
    if args['cutoff'] != args['cutoff'] or args['cutoff'] in (float('inf'), float('-inf')):
        _exit("--cutoff must be a finite number")
    if not 0 < args['core_frac'] <= 1:
        _exit("--core_frac must be above 0 and at most 1")
    if not 0 <= args['permutations'] <= 100000:
        _exit("--permutations must be between 0 and 100000")
    if args['seed'] < 0:
        _exit("--seed cannot be a negative number")
    if args['group_rows'] < 0:
        _exit("--group_rows cannot be a negative number")
    if args['chunk_bytes'] < 0:
        _exit("--chunk_bytes cannot be a negative number")
    if args['form'] not in (0, 1):
        _exit("--form must be 0 or 1")
    return args


COPYRIGHT = ["", "MIDAS: Metagenomic Intra-species Diversity Analysis System", "analysis commands on AMD Instinct MI355X (midas_amd %s)",
             "after github.com/snayfach/MIDAS, Copyright (C) 2015-2016 Stephen Nayfach",
             "Freely distributed under the GNU General Public License (GPLv3)", ""]


def print_copyright():
    import midas_amd
    sys.stdout.write('\n'.join(COPYRIGHT) % midas_amd.__version__ + '\n')
