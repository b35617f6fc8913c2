#!/usr/bin/env python
"""snp_pnps.py -- pN/pS per sample, gene or pool from one `merge_midas.py snps` directory, on MI355X.

The reference documents pN/pS as two snp_diversity.py runs (--locus_type CDS with --site_type 1D, then 4D) and the ratio of
their pi_bp.  This command makes both runs in one pass over the matrices (midas_amd/analyze/pnps.py) and writes both blocks of
columns and their ratio; each block is, byte for byte, what snp_diversity.py writes for that class.
"""
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

if __name__ == '__main__':
    from midas_amd.analyze import cli
    args = cli.pnps_arguments()
    cli.check_pnps_args(args)
    cli.print_copyright()
    cli.print_args(args, 'snp_pnps.py')
    from midas_amd.analyze import pnps
    pnps.run_pipeline(args)
