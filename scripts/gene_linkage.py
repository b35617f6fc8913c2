#!/usr/bin/env python
"""gene_linkage.py -- pairs of genes that are gained and lost together across samples, and the linkage groups they form, from
one `merge_midas.py genes` directory, on MI355X.  Not a command of the reference; its command line follows compare_genes.py.

The contract (the device call is midas_genes_linkage, midas_amd/csrc/genes_linkage.hip):

  rows      only genes_copynum.txt is read.  The header checks, --max_genes / --max_samples, the cell converter and the errors
            for a row of another width or a cell that is no finite decimal number are compare_genes.py's; an error is the
            earliest in file order, whatever the row groups are, and names file, line and column
  presence  gene g is present in sample s when value > --cutoff; c_g = the number of the S used samples in which g is present
  kept      g is kept when c_g >= --min_present and S - c_g >= --min_absent; kept genes get slots 0 .. K-1 in file order
  pairs     for kept slots a < b: both = popcount(P_a & P_b) over the ceil(S / 64) presence words (pad bits 0),
            either = c_a + c_b - both (>= 1, as --min_present >= 1); the pair is linked when
            (double)both / (double)either >= --min_jaccard, one fp64 division.  The division never runs on the device: the host
            builds need[u], u = 0 .. S, the smallest n in [0, u] with (double)n / (double)u >= --min_jaccard, by bisection over
            that very expression, and the kernel tests both >= need[either]
  output    the linked pairs (slot a, slot b, both) in ascending a, then ascending b, whatever --group_rows, --chunk_bytes or
            the kernel's tiles are.  More than --max_pairs linked pairs is an error that prints the exact total
  groups    label[k] = the smallest slot of the connected component of slot k in the graph of linked pairs (single linkage),
            computed on the device; a singleton has its own slot

  --out     gene1 gene2 count1 count2 count_both count_either jaccard, tab-separated, one row a linked pair in the order
            above; gene ids as in the file; jaccard is repr(float(both) / either)
  --groups  group_id group_size gene_id count: the kept genes of components with at least --min_group genes; group ids count
            from 1 in the order of each component's first gene; rows go by group id, then file order
"""
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

if __name__ == '__main__':
    from midas_amd.analyze import cli
    args = cli.gene_linkage_arguments()
    from midas_amd.analyze import genes_linkage
    genes_linkage.link(args)
