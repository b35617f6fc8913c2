#!/usr/bin/env python
"""merge_midas.py snps | genes -- multi-sample merges with the per-site / per-gene-cluster arithmetic on MI355X.

Drop-in for the `snps` and `genes` commands of the reference's scripts/merge_midas.py: same positional arguments, option
names, defaults, presets and output files (<outdir>/<species>/snps_{info,freq,depth,summary}.txt, readme.txt;
<outdir>/<species>/genes_{presabs,copynum,depth,reads,summary}.txt, readme.txt).  The option semantics are the
reference's (scripts/merge_midas.py:84-146, 148-281); the `species` merge is scripts/merge_species.py.  Under
torch.distributed.run the species are dealt to the ranks (one GPU each).
"""

import argparse
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

# preset flag -> the site filters it pins (applied in this order, later ones win, as in the reference)
PRESETS = [
    ('all_sites', dict(site_prev=0.0, snp_type=['any'])),
    ('all_snps', dict(site_prev=0.0, snp_type=['bi'])),
    ('core_sites', dict(site_depth=1, site_ratio=2.0, site_prev=0.95, snp_type=['any'])),
    ('core_snps', dict(site_depth=1, site_ratio=2.0, site_prev=0.95, snp_type=['bi'])),
]

OPTION_GROUPS = [
    ("Samples", [
        (['-i'], dict(dest='input', required=True, help="run_midas.py output directories; how to read this is set by -t")),
        (['-t'], dict(dest='intype', required=True, choices=['list', 'file', 'dir'], metavar='list|file|dir',
                      help="list: comma separated paths; file: one path per line; dir: every sub-directory")),
        (['-d'], dict(dest='db', default=os.environ.get('MIDAS_DB'), help="MIDAS reference database (default: $MIDAS_DB)")),
    ]),
    ("Presets", [
        (['--core_snps'], dict(action='store_true', help="bi-allelic sites present in >= 95 %% of the samples (the default behaviour)")),
        (['--core_sites'], dict(action='store_true', help="like --core_snps but keeps every site, variable or not")),
        (['--all_snps'], dict(action='store_true', help="bi-allelic sites, whatever their prevalence")),
        (['--all_sites'], dict(action='store_true', help="every site")),
    ]),
    ("Species", [
        (['--min_samples'], dict(type=int, default=1, metavar='INT', help="species found in at least this many samples (1)")),
        (['--species_id'], dict(metavar='ID[,ID...]', help="only these species")),
        (['--max_species'], dict(type=int, metavar='INT', help="at most this many species, most prevalent first")),
    ]),
    ("Sample filters, per species", [
        (['--sample_depth'], dict(type=float, default=5.0, metavar='FLOAT', help="minimum mean_coverage of the sample (5.0)")),
        (['--fract_cov'], dict(type=float, default=0.4, metavar='FLOAT', help="minimum fraction_covered of the sample (0.4)")),
        (['--max_samples'], dict(type=int, metavar='INT', help="use at most this many samples")),
        (['--all_samples'], dict(action='store_true', help="no sample filters (sample_depth = fract_cov = 0)")),
    ]),
    ("Site filters", [
        (['--snp_type'], dict(nargs='+', default=['bi'], choices=['any', 'mono', 'bi', 'tri', 'quad'], metavar='TYPE',
                              help="keep sites with 1/2/3/4 alleles at or above --allele_freq: mono bi tri quad, or any (bi)")),
        (['--allele_freq'], dict(type=float, default=0.01, metavar='FLOAT', help="pooled frequency at which an allele counts as present (0.01)")),
        (['--site_depth'], dict(type=int, default=1, metavar='INT', help="a sample passes at a site with at least this depth (1)")),
        (['--site_ratio'], dict(type=float, default=2.0, metavar='FLOAT', help="... and at most this depth / mean_coverage (2.0)")),
        (['--site_prev'], dict(type=float, default=0.95, metavar='FLOAT', help="keep sites where at least this fraction of samples passes (0.95)")),
        (['--max_sites'], dict(type=int, default=float('Inf'), metavar='INT', help="read only the first N sites of every table (all)")),
    ]),
]


def die(message):
    sys.exit("\nError: %s\n" % message)


def get_program():
    word = sys.argv[1] if len(sys.argv) > 1 else '-h'
    if word in ('-h', '--help'):
        print("merge_midas.py <command> [options]\n\n"
              "  snps   pool the per-sample allele counts of a species, call alleles and SNP types, write the\n"
              "         freq/depth/info matrices (site arithmetic on the MI355X); `merge_midas.py snps -h` for options\n"
              "  genes  merge the per-sample gene tables of a species over its gene clusters, write the presence/absence,\n"
              "         copy-number, depth and read matrices (cluster sums on the MI355X); `merge_midas.py genes -h` for options\n\n"
              "the species merge is a script of its own: merge_species.py OUT -i INPUT -t list|file|dir (`merge_species.py -h`).")
        sys.exit(0)
    if word == 'species':
        die("'%s' is not part of this build (only the snps and genes paths are)" % word)
    if word not in ('snps', 'genes'):
        die("Unrecognized command: '%s'" % word)
    return word


def add_snp_presets(args):
    """--all_samples and the four presets overwrite the individual filters (scripts/merge_midas.py:259-281)."""
    if args['all_samples']:
        args['sample_depth'] = args['fract_cov'] = 0.0
    for flag, pinned in PRESETS:
        if args[flag]:
            args.update({k: (list(v) if isinstance(v, list) else v) for k, v in pinned.items()})
    return args


def snps_arguments():
    parser = argparse.ArgumentParser(
        prog='merge_midas.py snps', formatter_class=argparse.RawTextHelpFormatter,
        description="Multi-sample SNP calling over the core genome of each species.",
        epilog="examples:\n"
               "  merge_midas.py snps OUT -i sample_1,sample_2 -t list\n"
               "  merge_midas.py snps OUT -i /path/to/samples -t dir --core_sites")
    parser.add_argument('program', help=argparse.SUPPRESS)
    parser.add_argument('outdir', help="output directory; one sub-directory per species")
    parser.add_argument('--threads', type=int, default=1, metavar='INT', help="CPU threads for reading and writing tables (1)")
    for title, options in OPTION_GROUPS:
        group = parser.add_argument_group(title)
        for flags, kw in options:
            group.add_argument(*flags, **kw)
    return add_snp_presets(vars(parser.parse_args()))


GENES_OPTION_GROUPS = [
    ("Samples", OPTION_GROUPS[0][1]),
    ("Species", OPTION_GROUPS[2][1]),
    ("Sample filters, per species", [
        (['--sample_depth'], dict(type=float, default=1.0, metavar='FLOAT',
                                  help="minimum mean_coverage (read depth over the genes with reads) of the sample (1.0)")),
        (['--max_samples'], dict(type=int, metavar='INT', help="use at most this many samples")),
    ]),
    ("Quantification", [
        (['--cluster_pid'], dict(type=str, dest='cluster_pid', default='95', choices=['75', '80', '85', '90', '95', '99'],
                                 help="the pangenome's gene clusters at this %% identity: 75 80 85 90 95 99 (95)")),
        (['--min_copy'], dict(type=float, default=0.35, metavar='FLOAT',
                              help="a cluster is present (1) at or above this copy number, absent (0) below (0.35)")),
    ]),
]


def genes_arguments():
    parser = argparse.ArgumentParser(
        prog='merge_midas.py genes', formatter_class=argparse.RawTextHelpFormatter,
        description="Gene-cluster presence/absence, copy-number, depth and read matrices over the samples of each species.",
        epilog="examples:\n"
               "  merge_midas.py genes OUT -i sample_1,sample_2 -t list\n"
               "  merge_midas.py genes OUT -i /path/to/samples -t dir --sample_depth 5.0 --min_copy 0.1")
    parser.add_argument('program', help=argparse.SUPPRESS)
    parser.add_argument('outdir', help="output directory; one sub-directory per species")
    parser.add_argument('--threads', type=int, default=1, metavar='INT', help="CPU threads for reading and writing tables (1)")
    for title, options in GENES_OPTION_GROUPS:
        group = parser.add_argument_group(title)
        for flags, kw in options:
            group.add_argument(*flags, **kw)
    return vars(parser.parse_args())


def check_arguments(args):
    """scripts/merge_midas.py:283-332, the parts that apply to snps and genes."""
    os.makedirs(args['outdir'], exist_ok=True)
    if args['db'] is None:
        die("No reference database specified\nUse the flag -d to specify a database,\n"
            "Or set the MIDAS_DB environmental variable: export MIDAS_DB=/path/to/midas/db")
    if not os.path.isdir(args['db']):
        die("Specified reference database does not exist: %s" % args['db'])
    kind, source = args['intype'], args['input']
    if kind == 'dir':
        if not os.path.isdir(source):
            die("Specified input directory '%s' does not exist" % source)
        # every entry is taken, as in the reference (a stray README or tarball among the samples is dropped later,
        # when it turns out to have no snps/summary.txt); sorted, so that the sample columns do not depend on the
        # file system's listing order
        args['indirs'] = [os.path.join(source, d) for d in sorted(os.listdir(source))]
    else:
        if kind == 'file':
            if not os.path.isfile(source):
                die("Specified input file '%s' does not exist" % source)
            with open(source) as handle:
                args['indirs'] = [line.strip().rstrip('/') for line in handle if line.strip()]
        else:
            args['indirs'] = source.split(',')
        for d in args['indirs']:      # only listed directories are checked (scripts/merge_midas.py:320-331)
            if not os.path.isdir(d):
                die("Specified input directory '%s' does not exist" % d)
    if args.get('program') in ('genes', 'species'):       # (species: scripts/merge_species.py)
        for name in ('min_copy', 'sample_depth', 'max_samples'):       # scripts/merge_midas.py:295-298
            if args.get(name) and args[name] < 0:
                die("--%s cannot be a negative value" % name)
        return
    if args['site_depth'] < 0:
        die("--site_depth must be >=0")
    for name in ('allele_freq', 'fract_cov', 'site_prev'):      # scripts/merge_midas.py:291-293
        if args.get(name) and not 0.0 <= args[name] <= 1.0:
            die("--%s must be between 0.0 and 1.0" % name)
    if args['max_sites'] != float('Inf') and args['max_sites'] < 0:
        die("--max_sites must be >= 0")


if __name__ == '__main__':
    program = get_program()
    args = snps_arguments() if program == 'snps' else genes_arguments()
    check_arguments(args)
    if program == 'snps':
        from midas_amd.merge import snps
        snps.run_pipeline(args)
    else:
        from midas_amd.merge import genes
        genes.run_pipeline(args)
