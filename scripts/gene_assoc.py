#!/usr/bin/env python
"""gene_assoc.py -- the genes of a pangenome whose presence or copy number differs between two groups of samples (case /
control, two sites, before / after), with a permutation test, from one `merge_midas.py genes` directory, on MI355X.  Not a
command of the reference; its command line follows compare_genes.py.

The contract is DESIGN.md section 22 (the device call is midas_genes_assoc, midas_amd/csrc/genes_assoc.hip): the rows are read
under compare_genes.py's rules; --groups holds lines of sample_id<TAB>label with two distinct labels among the samples of the
matrix; presabs is Fisher's exact test on the presence counts, copynum the rank-sum test on the doubled midranks; p_perm comes
from --permutations relabellings of the samples, formed on the device as an exact i8 matrix product; q is Benjamini-Hochberg.

  --out     gene_id count_case count_control effect p_value q_value [exceed p_perm q_perm], tab-separated, one row a kept gene in
            matrix order; floats as str() writes them
"""
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

if __name__ == '__main__':
    from midas_amd.analyze import cli
    args = cli.gene_assoc_arguments()
    from midas_amd.analyze import genes_assoc
    genes_assoc.assoc(args)
