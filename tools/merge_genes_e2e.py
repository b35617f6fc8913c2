"""`merge_midas.py genes` end to end on synthetic inputs, phase by phase.

Writes S sample tables of G genes each (default 200 x 300 000, every table listing the pangenome's genes in sorted order, as
run_midas.py genes writes them) and a gene_info.txt (three genes a 95 % cluster) on tmpfs, then runs the species' merge as
merge_midas.py does and prints where the time goes: gene_info read, tables read, resolve, the device call (upload + kernels +
download) with the kernels' own time, and the four writers.  The kernels' algorithmic bytes: per sample the three
columns read once (24 B a row) and the four outputs written (25 B a cell) -- reported as a fraction of 8 TB/s.

usage: python tools/merge_genes_e2e.py [--samples 200] [--genes 300000] [--threads 16] [--dir /dev/shm] [--keep]
"""
import argparse
import gzip
import os
import shutil
import sys
import tempfile
import time
import types
from concurrent.futures import ProcessPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from midas_amd import abi  # noqa: E402
from midas_amd.merge import genes  # noqa: E402


def _write_sample(job):
    path, ids, seed = job
    rng = np.random.default_rng(seed)
    n = len(ids)
    reads = rng.integers(0, 3000, n)
    cov = rng.random(n) * 40.0
    cp = cov / 11.7
    cp[rng.random(n) < 0.2] = 0.0
    lines = ['gene_id\tcount_reads\tcoverage\tcopy_number']
    lines += ['%s\t%d\t%r\t%r' % t for t in zip(ids, reads.tolist(), cov.tolist(), cp.tolist())]
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with gzip.open(path, 'wb', compresslevel=1) as h:
        h.write(('\n'.join(lines) + '\n').encode())
    return path


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--samples', type=int, default=200)
    ap.add_argument('--genes', type=int, default=300000)
    ap.add_argument('--threads', type=int, default=16)
    ap.add_argument('--group', type=int, default=0, help="samples on the device at a time (0: the library's budget)")
    ap.add_argument('--dir', default='/dev/shm' if os.path.isdir('/dev/shm') else None)
    ap.add_argument('--keep', action='store_true')
    a = ap.parse_args()
    root = tempfile.mkdtemp(prefix='merge_genes_e2e_', dir=a.dir)
    try:
        sp = 'Species_00001'
        ids = sorted('%s.peg.%d' % (sp[-5:], k) for k in range(a.genes))
        t0 = time.perf_counter()
        db = os.path.join(root, 'db')
        os.makedirs(os.path.join(db, 'pan_genomes', sp))
        with open(os.path.join(db, 'pan_genomes', sp, 'gene_info.txt'), 'w') as h:
            h.write('gene_id\tgenome_id\tcentroid_99\tcentroid_95\n')
            h.write(''.join('%s\t%s.rep\t%s\t%s\n' % (g, sp, g, ids[k - k % 3]) for k, g in enumerate(ids)))
        jobs = [(os.path.join(root, 's%04d' % s, 'genes', 'output', sp + '.genes.gz'), ids, s) for s in range(a.samples)]
        with ProcessPoolExecutor(min(16, a.threads)) as ex:
            list(ex.map(_write_sample, jobs, chunksize=1))
        print("inputs: %d samples x %d genes written in %.1f s (%s)" % (a.samples, a.genes, time.perf_counter() - t0, root))
        species = types.SimpleNamespace(id=sp, samples=[types.SimpleNamespace(id='s%04d' % s, dir=os.path.join(root, 's%04d' % s))
                                                        for s in range(a.samples)])
        args = dict(outdir=os.path.join(root, 'out'), db=db, cluster_pid='95', min_copy=0.35, threads=a.threads, group_samples=a.group)
        with abi.Context(0) as ctx:
            ctx.genes_merge([np.zeros(1, np.uint32)], [np.zeros(1)], [np.zeros(1)], [np.zeros(1, np.int64)], 1, 0.35)   # warm
            t = {}
            w0 = time.perf_counter()
            rows, n_clusters = genes.merge_species(species, args, ctx, t)
            wall = time.perf_counter() - w0
        S, G = a.samples, a.genes
        alg = S * (G * 24 + rows * 25)
        ks = t['kernel_ms'] / 1e3
        print("clusters %d, rows %d, samples %d" % (n_clusters, rows, S))
        for k in ('gene_info', 'tables', 'resolve', 'merge', 'write_presabs', 'write_copynum', 'write_depth', 'write_reads'):
            print("  %-14s %8.3f s" % (k, t[k]))
        print("  %-14s %8.3f s  (kernels, inside merge; upload + download + host: %.3f s)" % ('kernels', ks, t['merge'] - ks))
        print("  %-14s %8.3f s" % ('total', wall))
        print("kernel algorithmic bytes %.3f GB: %.1f GB/s = %.2f %% of 8 TB/s" % (alg / 1e9, alg / ks / 1e9 if ks else 0.0,
                                                                                   100.0 * alg / ks / 8e12 if ks else 0.0))
        out = sum(os.path.getsize(os.path.join(args['outdir'], sp, 'genes_%s.txt' % m)) for m in genes.MATRICES)
        print("matrices: %.1f MB" % (out / 1e6))
    finally:
        if not a.keep:
            shutil.rmtree(root, ignore_errors=True)


if __name__ == '__main__':
    main()
