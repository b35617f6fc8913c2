#!/usr/bin/env python
"""snp_trees.py -- a neighbour-joining tree of the samples of one `merge_midas.py snps` directory, on MI355X.

The whole of the reference's docs/snp_trees.md in one command: the consensus calls of call_consensus.py (same sample and site
options), the pairwise distances over them (--dist) and the tree in Newick format (--out).  The matrices are parsed, the calls
compared and the tree joined on the device (midas_amd/analyze/trees.py).
"""
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

if __name__ == '__main__':
    from midas_amd.analyze import cli
    args = cli.trees_arguments()
    cli.check_trees_args(args)
    cli.print_copyright()
    cli.print_trees_args(args)
    from midas_amd.analyze import trees
    trees.run_pipeline(args)
