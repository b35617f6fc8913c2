#!/usr/bin/env python
"""snp_diversity.py -- nucleotide diversity and SNP density from one `merge_midas.py snps` directory, on MI355X.

Drop-in for the reference's scripts/snp_diversity.py: same positional argument, option names, defaults and output table.
The matrices are parsed and reduced on the device (midas_amd/analyze/diversity.py), --rand_reads / --replace_reads included:
the device continues numpy's own random stream.  --seed INT (not in the reference) seeds both global streams first.
"""
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

if __name__ == '__main__':
    from midas_amd.analyze import cli
    args = cli.diversity_arguments()
    cli.check_diversity_args(args, resampling=True)
    cli.print_copyright()
    cli.print_args(args, 'snp_diversity.py')
    from midas_amd.analyze import diversity
    diversity.run_pipeline(args)
