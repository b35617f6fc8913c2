#!/usr/bin/env python
"""gene_curves.py -- how the pangenome of one species grows and its core genome shrinks as samples are added (accumulation or
rarefaction curves, with Heaps' law for "open or closed"), from one `merge_midas.py genes` directory, on MI355X.  Not a command
of the reference; its command line follows compare_genes.py.

The contract is DESIGN.md section 23 (the device call is midas_genes_curves, midas_amd/csrc/genes_curves.hip): the rows are read
under compare_genes.py's rules; a gene is present in a sample when its copy number > --cutoff; for the listed order of the
samples in use (all, or those of --samples) and for --permutations random orders (numpy's default_rng(--seed)), c = the number
of the first k samples in which a gene is present, and pan counts the genes with c >= 1, core those with c >= need[k], single
those with c == 1, where need[k] is the smallest n >= 1 with float(n) / float(k) >= --core_frac.

  --out     samples pan core single new [pan_mean pan_min pan_max core_mean core_min core_max single_mean single_min single_max
            new_mean], tab-separated, one row a k = 1 .. N; the first five from the listed order, the statistics over the random
            orders (left out with --permutations 0); floats as str() writes them
  --orders  order samples sample_id pan core single, one row an order (0: the listed one) and k
  stdout    rows read, samples in use, orders and seed, pan / core / single of all N samples, and Heaps' law fitted to the mean
            new genes a sample: new ~ K k^-alpha, open when alpha <= 1
"""
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

if __name__ == '__main__':
    from midas_amd.analyze import cli
    args = cli.gene_curves_arguments()
    from midas_amd.analyze import genes_curves
    genes_curves.curves(args)
