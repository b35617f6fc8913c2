#!/usr/bin/env python
"""merge_species.py OUT -i INPUT -t list|file|dir [options] -- species abundance matrices and prevalence over samples, on MI355X.

Serves what `merge_midas.py species` serves in the reference: same options, defaults, checks and output files
(<outdir>/{relative_abundance,coverage,count_reads,species_prevalence,readme}.txt).  The samples' species/species_profile.txt
files are parsed, scattered into [species][sample] matrices and reduced per species on the GPU; the matrices are byte for byte
what the reference writes.  A profile the reference would take silently wrong (an unknown or missing or repeated species, a cell
that is no number) is an error here that names the file and the line.
"""

import argparse
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, 'scripts'))

import merge_midas  # noqa: E402  (the sample listing and the argument checks of the snps and genes merges)


def build_parser():
    parser = argparse.ArgumentParser(
        prog='merge_species.py', formatter_class=argparse.RawTextHelpFormatter,
        description="Merge species abundance files across samples:\n"
                    "  relative_abundance.txt, coverage.txt, count_reads.txt   a row a species of species_info.txt, a column a sample\n"
                    "  species_prevalence.txt   mean and median coverage and abundance, and in how many samples the species\n"
                    "                           reaches --sample_depth; most prevalent first\n"
                    "Input: sample directories written by run_species.py (or the reference's run_midas.py species).",
        epilog="examples:\n"
               "  merge_species.py OUT -i sample_1,sample_2 -t list\n"
               "  merge_species.py OUT -i /path/to/samples -t dir\n"
               "  merge_species.py OUT -i sample_paths.txt -t file --max_samples 2")
    parser.add_argument('outdir', help="directory for the output files (created if absent)")
    parser.add_argument('-i', dest='input', required=True, help="sample directories; how to read this is set by -t")
    parser.add_argument('-t', dest='intype', required=True, choices=['list', 'file', 'dir'], metavar='list|file|dir',
                        help="list: comma separated paths; file: one path per line; dir: every sub-directory (sorted)")
    parser.add_argument('-d', dest='db', default=os.environ.get('MIDAS_DB'), help="MIDAS reference database (default: $MIDAS_DB)")
    parser.add_argument('--sample_depth', type=float, default=1.0, metavar='FLOAT',
                        help="minimum per-sample marker-gene depth for estimating species prevalence (1.0)")
    parser.add_argument('--max_samples', type=int, metavar='INT', help="use at most this many samples (all)")
    parser.add_argument('--profile', action='store_true', help="print the phases of the merge and their times")
    return parser


def print_arguments(args):
    print("===========Parameters===========")
    print("Command: %s" % ' '.join(sys.argv))
    print("Script: merge_species.py (MI355X)")
    print("Database: %s" % args['db'])
    print("Input: %s" % args['input'])
    print("Input type: %s" % args['intype'])
    print("Output directory: %s" % args['outdir'])
    print("Minimum coverage for estimating prevalence: %s" % args['sample_depth'])
    if args['max_samples']:
        print("Keep <= %s samples" % args['max_samples'])
    print("===============================")
    print("")


if __name__ == '__main__':
    args = vars(build_parser().parse_args())
    args['program'] = 'species'
    merge_midas.check_arguments(args)
    print_arguments(args)
    from midas_amd.merge import species
    species.run_pipeline(args)
