"""MI355X-native `merge_midas.py genes`: the host side.

Mirrors /root/reference/midas/merge/genes.py: same outputs (<outdir>/<species>/genes_{presabs,copynum,depth,reads}.txt,
genes_summary.txt, readme.txt), same rows and cells.  Underneath: the cluster map (read_cluster_map, :91-98) and the sample
tables are read natively (abi.GeneClusterMap / abi.GeneTables, one worker per file), the per-row dict updates of
build_gene_matrices (:12-30) run on the GPU for every (cluster, sample) at once (midas_genes_merge: fp64 sums in table row
order, as the reference adds), and write_gene_matrices' str() of every cell (:32-48) is the native writer's.  No CPU fallback
for the arithmetic.
"""

import os
import sys
import time

from midas_amd import abi, dist
from midas_amd.merge import merge

MATRICES = ('presabs', 'copynum', 'depth', 'reads')
RESULT_OF = {'presabs': 'state', 'copynum': 'copy', 'depth': 'depth', 'reads': 'reads'}


def gene_info_path(db, species_id):
    """DB/pan_genomes/<sp>/gene_info.txt[.gz]: the .gz wins when both exist (genes.py:93-96)."""
    found = None
    for ext in ('', '.gz'):
        path = '/'.join([db, 'pan_genomes', species_id, 'gene_info.txt%s' % ext])
        if os.path.isfile(path):
            found = path
    if found is None:
        sys.exit("\nError: no gene_info.txt[.gz] for species %s under %s/pan_genomes\n" % (species_id, db))
    return found


def _table_paths(species):
    return ['%s/genes/output/%s.genes.gz' % (s.dir, species.id) for s in species.samples]


def merge_species(species, args, ctx, timings=None):
    """read_cluster_map + build_gene_matrices + write_gene_matrices (genes.py:12-48, 91-98) for one species.
    timings (dict, optional): seconds per phase."""
    t = timings if timings is not None else {}
    threads = int(args.get('threads', 1) or 1)
    outdir = os.path.join(args['outdir'], species.id)
    os.makedirs(outdir, exist_ok=True)
    paths = _table_paths(species)
    for p in paths:
        if not os.path.isfile(p):
            sys.exit("\nError: missing genes table %s\n" % p)
    t0 = time.perf_counter()
    try:
        cmap = abi.GeneClusterMap(gene_info_path(args['db'], species.id), 'centroid_%s' % args['cluster_pid'])
        t1 = time.perf_counter()
        tables = abi.GeneTables(paths, threads)
        t2 = time.perf_counter()
        tables.resolve(cmap, reuse=True, threads=threads)
        t3 = time.perf_counter()
    except abi.MidasSnpsError as e:
        sys.exit("\nError: %s\n" % e.message)
    res = ctx.genes_merge(tables.cluster, tables.copy, tables.depth, tables.reads, cmap.n_clusters, float(args['min_copy']),
                          int(args.get('group_samples', 0) or 0))
    t4 = time.perf_counter()
    t.update(gene_info=t1 - t0, tables=t2 - t1, resolve=t3 - t2, merge=t4 - t3, kernel_ms=res.get('kernel_ms', 0.0))
    header = '\t'.join(['gene_id'] + [s.id for s in species.samples]) + '\n'
    for name in MATRICES:
        w0 = time.perf_counter()
        abi.write_genes_matrix('%s/genes_%s.txt' % (outdir, name), header, name, res['rows'], cmap, res[RESULT_OF[name]],
                               res['state'], threads=threads)
        t['write_' + name] = time.perf_counter() - w0
    return len(res['rows']), cmap.n_clusters


README = """merge_midas.py genes -- files in this directory (species %s)

The samples' gene tables (run_midas.py genes) merged over the pangenome's gene clusters at %s %% identity: every gene of
a table counts towards its cluster.  One row per cluster that the first sample's table mentions, sorted by cluster id; one
column per sample, in input order.

genes_copynum.txt  per sample the sum of the cluster's gene copy numbers (read depth over the median depth of the
                   universal single-copy genes)
genes_depth.txt    per sample the sum of the cluster's gene read depths
genes_reads.txt    per sample the sum of the reads mapped to the cluster's genes
genes_presabs.txt  per sample 1 when the copy number is at least %s, 0 when it is below; a cluster the sample's table
                   does not list reads 0.0 here and 0.0 / 0.0 / 0 in the three matrices above
genes_summary.txt  the samples' own summary rows for this species (from run_midas.py genes): pangenome_size,
                   covered_genes, fraction_covered, mean_coverage, marker_coverage, aligned_reads, mapped_reads

Pangenome and gene clusters of the species: %s/pan_genomes/%s
"""


def write_genes_readme(args, sp):
    with open('%s/%s/readme.txt' % (args['outdir'], sp.id), 'w') as handle:
        handle.write(README % (sp.id, args['cluster_pid'], args['min_copy'], args['db'], sp.id))


def _device_context():
    return abi.Context(int(os.environ.get("LOCAL_RANK", "0")))


class _LazyContext:
    """The device context, opened by the first merge: a species whose inputs fail to read stops before the GPU is touched."""

    def __init__(self, make_context):
        self._make, self._ctx = make_context, None

    def genes_merge(self, *a, **kw):
        if self._ctx is None:
            self._ctx = self._make()
        return self._ctx.genes_merge(*a, **kw)

    def close(self):
        if self._ctx is not None:
            self._ctx.close()
            self._ctx = None


def run_pipeline(args, make_context=_device_context):
    """midas/merge/genes.py:100-131.  N ranks: species k goes to rank k mod N, which writes its directory; the ranks
    exchange nothing but "still standing" flags.  make_context: tests substitute a CPU double of the device."""
    rank, ws = dist.init_from_env(rendezvous_dir=args['outdir'])
    if rank == 0:
        print("Identifying species and samples")
    species_list = merge.select_species(args, dtype='genes')
    if rank == 0:
        for species in species_list:
            print("  %s" % species.id)
            print("    count genomes: %s" % species.info.get('count_genomes', 'NA'))
            print("    count samples: %s" % len(species.samples))
        print("\nMerging genes")
    error = None
    try:        # a rank that fails takes the others down with it at the end, instead of leaving them at the barrier
        ctx = _LazyContext(make_context)
        try:
            for k, species in enumerate(species_list):
                if k % ws != rank:
                    continue
                print("  %s" % species.id)
                print("    building pangenome matrices")
                timings = {}
                rows, n_clusters = merge_species(species, args, ctx, timings)
                print("    %d clusters, %d rows (%.3f ms on the GPU)" % (n_clusters, rows, timings['kernel_ms']))
                print("    writing summary statistics")
                species.write_sample_info(dtype='genes', outdir=args['outdir'])
                write_genes_readme(args, species)
                print("    done!")
        finally:
            ctx.close()
    except abi.MidasSnpsError as e:
        error = "\nError: %s\n" % e.message
    except SystemExit as e:
        error = dist.exit_message(e)
    except Exception as e:      # (an OSError, a MemoryError ...: the other ranks must not wait for this one)
        error = "\nError: %s: %s\n" % (type(e).__name__, e)
    dist.agree_or_exit(error)
    dist.barrier()
    dist.finalize()
