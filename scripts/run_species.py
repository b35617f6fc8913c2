#!/usr/bin/env python
"""run_species.py OUT [options] -- species abundance of a metagenome from reads mapped to the marker genes, on MI355X.

Serves what `run_midas.py species` serves in the reference: same options, ranges, messages and output layout
(<outdir>/species/{species_profile.txt, log.txt, temp/}).  The reads go through hs-blastn (from PATH); its m8 lines are
parsed, filtered, grouped by read and reduced to best hits on the GPU; the reads whose best hits tie are assigned by the
reference's serial weighted draw on the host.  Two options are added: --classify takes an existing
species/temp/alignments.m8 and skips the aligner, --seed seeds both generators the draws use.
"""

import argparse
import os
import platform
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from midas_amd import utility  # noqa: E402


def build_parser():
    parser = argparse.ArgumentParser(
        prog='run_species.py', formatter_class=argparse.RawTextHelpFormatter,
        description="Map reads to the database of phylogenetic marker genes and estimate species abundance:\n"
                    "  1) align the reads to the marker genes with hs-blastn\n"
                    "  2) assign reads to species with the marker families' identity cutoffs (this is the GPU stage)\n"
                    "  3) assign reads that map equally well to several species by weighted draws\n"
                    "  4) sequencing depth and relative abundance per species\n"
                    "Afterwards: run_midas.py snps / genes with --species_cov or --species_topn.",
        epilog="examples:\n"
               "  run_species.py OUT -1 reads_1.fq.gz -2 reads_2.fq.gz\n"
               "  run_species.py OUT -1 reads_1.fq.gz -t 4 -n 4000000\n"
               "  run_species.py OUT --classify --seed 1")
    parser.add_argument('outdir', help="sample directory (its name is the sample id)")
    parser.add_argument('-1', dest='m1', help="FASTA/FASTQ of unpaired reads or of the first mates (.gz / .bz2 accepted); required unless --classify")
    parser.add_argument('-2', dest='m2', help="FASTA/FASTQ of the second mates")
    parser.add_argument('-n', dest='max_reads', type=int, help="use only the first N reads (all)")
    parser.add_argument('-t', dest='threads', default=1, help="threads for the database search (1)")
    parser.add_argument('-d', dest='db', default=os.environ.get('MIDAS_DB'), help="MIDAS reference database (default: $MIDAS_DB)")
    parser.add_argument('--remove_temp', action='store_true', help="delete <outdir>/species/temp when done")
    parser.add_argument('--word_size', type=int, metavar='INT', default=28, help="word size of the search (28)")
    parser.add_argument('--mapid', type=float, metavar='FLOAT', help="drop alignments below this identity (default: the marker family's own cutoff)")
    parser.add_argument('--aln_cov', type=float, metavar='FLOAT', default=0.75, help="drop alignments over less than this fraction of the read (0.75)")
    parser.add_argument('--read_length', type=int, metavar='INT', help="cut reads to this length and drop shorter ones (off)")
    parser.add_argument('--classify', action='store_true', help="classify the existing <outdir>/species/temp/alignments.m8; no aligner is run")
    parser.add_argument('--seed', type=int, metavar='INT', help="random.seed(INT) and numpy.random.seed(INT) before the draws (default: as the interpreter seeded them)")
    return parser


def check_arguments(args):
    """The reference's check_species (scripts/run_midas.py:170-193): same conditions, same exits."""
    if not args['classify'] and not args['m1']:
        build_parser().error("the following arguments are required: -1")
    if args['m1'] and not args['classify']:
        if not os.path.isfile(args['m1']):
            sys.exit("\nError: Input file does not exist: '%s'\n" % args['m1'])
        args['file_type'] = utility.auto_detect_file_type(args['m1'])
    utility.check_database(args)
    os.makedirs(os.path.join(args['outdir'], 'species'), exist_ok=True)
    if args['word_size'] < 12:
        sys.exit("\nError: Invalid word size: %s. Must be greater than or equal to 12\n" % args['word_size'])
    if args['mapid'] and (args['mapid'] < 0 or args['mapid'] > 100):
        sys.exit("\nError: Invalid mapping identity: %s. Must be between 0 and 100\n" % args['mapid'])
    if args['aln_cov'] < 0 or args['aln_cov'] > 1:
        sys.exit("\nError: Invalid alignment coverage: %s. Must be between 0 and 1\n" % args['aln_cov'])
    if not args['classify']:
        for key in ('m1', 'm2'):
            if args[key] and not os.path.isfile(args[key]):
                sys.exit("\nError: Input file does not exist: '%s'\n" % args[key])
        for key in ('m1', 'm2'):
            if args[key]:
                utility.check_compression(args[key])
        if not args['hs-blastn']:
            sys.exit("\nError: hs-blastn not found on PATH (needed to align; the aligner is not part of this build)\n")
    elif not os.path.isfile(os.path.join(args['outdir'], 'species', 'temp', 'alignments.m8')):
        sys.exit("\nError: You've specified --classify, but no alignments were found: %s\n"
                 % os.path.join(args['outdir'], 'species', 'temp', 'alignments.m8'))
    if platform.system() not in ('Linux', 'Darwin'):
        sys.exit("\nError: Operating system '%s' not supported\n" % platform.system())


def print_arguments(args):
    lines = ["===========Parameters===========", "Command: %s" % ' '.join(sys.argv), "Script: run_species.py (MI355X)",
             "Database: %s" % args['db'], "Output directory: %s" % args['outdir']]
    if args['classify']:
        lines.append("Alignments: species/temp/alignments.m8 (--classify)")
    elif args['m2']:
        lines += ["Input reads (1st mate): %s" % args['m1'], "Input reads (2nd mate): %s" % args['m2']]
    else:
        lines.append("Input reads (unpaired): %s" % args['m1'])
    lines += ["Remove temporary files: %s" % args['remove_temp'], "Word size for database search: %s" % args['word_size']]
    if args['mapid']:
        lines.append("Minimum mapping identity: %s" % args['mapid'])
    lines += ["Minimum mapping alignment coverage: %s" % args['aln_cov'],
              "Number of reads to use from input: %s" % (args['max_reads'] if args['max_reads'] else 'use all')]
    if args['read_length']:
        lines.append("Trim reads from 3'/right end to %s-bp and discard reads with length < %s-bp" % (args['read_length'], args['read_length']))
    lines.append("Number of threads for database search: %s" % args['threads'])
    if args['seed'] is not None:
        lines.append("Seed of the draws: %s" % args['seed'])
    lines.append("================================")
    args['log'].write('\n'.join(lines) + '\n')
    sys.stdout.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    args = vars(build_parser().parse_args())
    args['hs-blastn'] = utility.find_executable('hs-blastn')
    check_arguments(args)
    for sub in ('', 'temp'):
        os.makedirs(os.path.join(args['outdir'], 'species', sub), exist_ok=True)
    args['log'] = open(os.path.join(args['outdir'], 'species', 'log.txt'), 'w')
    print_arguments(args)
    from midas_amd.run import species
    species.run_pipeline(args)
    args['log'].close()
