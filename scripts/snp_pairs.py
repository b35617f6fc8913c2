#!/usr/bin/env python
"""snp_pairs.py -- pooled diversity, dxy and Fst of every pair of samples from one `merge_midas.py snps` directory, on MI355X.

The reference gives between-sample heterogeneity as `snp_diversity.py --sample_type pooled-samples`, one number for the pool;
which samples differ takes one run per pair with --keep_samples a,b.  This command makes all of these runs in one pass over the
matrices (midas_amd/analyze/pairs.py): the pooled columns of every row are, byte for byte, what that run writes for the pair.
"""
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

if __name__ == '__main__':
    from midas_amd.analyze import cli
    args = cli.pairs_arguments()
    cli.check_pairs_args(args)
    cli.print_copyright()
    cli.print_args(args, 'snp_pairs.py')
    from midas_amd.analyze import pairs
    pairs.run_pipeline(args)
