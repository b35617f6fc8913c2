#!/usr/bin/env python
"""compare_genes.py -- gene-content distances between all pairs of samples, from one `merge_midas.py genes` directory, on
MI355X.

Drop-in for the reference's scripts/compare_genes.py: its option names, defaults, progress lines and output table, byte for
byte.  The matrix is parsed and every pair is summed on the device (midas_amd/analyze/genes_compare.py).
"""
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

if __name__ == '__main__':
    from midas_amd.analyze import cli
    args = cli.compare_genes_arguments()
    from midas_amd.analyze import genes_compare
    genes_compare.compare(args)
