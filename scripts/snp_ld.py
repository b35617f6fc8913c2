#!/usr/bin/env python
"""snp_ld.py -- linkage disequilibrium between the sites of one `merge_midas.py snps` directory, by distance, on MI355X.

The consensus calls of call_consensus.py (same sample and site options); for every pair of retained sites at most --max_dist
bases apart, r2 and the terms of sigma2_d over the samples called at both; one row per distance bin (--out).  The matrices are
parsed, the calls kept and the pairs of sites visited on the device (midas_amd/analyze/ld.py).
"""
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

if __name__ == '__main__':
    from midas_amd.analyze import cli
    args = cli.ld_arguments()
    cli.check_ld_args(args)
    cli.print_copyright()
    cli.print_ld_args(args)
    from midas_amd.analyze import ld
    ld.run_pipeline(args)
