"""Test-side helpers for `merge_midas.py genes`: a numpy double of Context.genes_merge (sequential fp64 sums in table row
order: np.add.at adds an index's terms one after the other, in index order) and the on-disk layout of
tests/golden/merge_genes_vectors.json (a MIDAS DB with pan_genomes/<sp>/gene_info.txt[.gz] and the sample directories)."""
import base64
import gzip
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
MATRICES = ('presabs', 'copynum', 'depth', 'reads')
SUMMARY_FIELDS = ('pangenome_size', 'covered_genes', 'fraction_covered', 'mean_coverage', 'marker_coverage', 'aligned_reads',
                  'mapped_reads')


def model_merge(cluster, copy, depth, reads, n_clusters, min_copy):
    C, S = int(n_clusters), len(cluster)
    cl = [np.asarray(c, dtype=np.int64) for c in cluster]
    present0 = np.zeros(C, bool)
    present0[cl[0]] = True
    rows = np.nonzero(present0)[0]
    R = rows.shape[0]
    out = dict(rows=rows.astype(np.uint32), copy=np.zeros((R, S)), depth=np.zeros((R, S)), reads=np.zeros((R, S), np.int64),
               state=np.zeros((R, S), np.uint8))
    for s in range(S):
        c, d = np.zeros(C), np.zeros(C)
        r = np.zeros(C, np.int64)
        np.add.at(c, cl[s], np.asarray(copy[s], np.float64))
        np.add.at(d, cl[s], np.asarray(depth[s], np.float64))
        np.add.at(r, cl[s], np.asarray(reads[s], np.int64))
        n = np.bincount(cl[s], minlength=C)
        out['copy'][:, s], out['depth'][:, s], out['reads'][:, s] = c[rows], d[rows], r[rows]
        with np.errstate(invalid='ignore'):
            out['state'][:, s] = np.where(n[rows] > 0, np.where(c[rows] >= min_copy, 2, 1), 0)
    out['kernel_ms'] = 0.0
    return out


class NumpyGenesContext:
    """What run_pipeline's make_context may return in place of abi.Context: genes_merge on the CPU."""

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def close(self):
        pass

    def genes_merge(self, cluster, copy, depth, reads, n_clusters, min_copy, group_samples=0):
        return model_merge(cluster, copy, depth, reads, n_clusters, min_copy)


def load_vectors():
    with open(os.path.join(HERE, 'golden', 'merge_genes_vectors.json')) as h:
        return json.load(h)


def write_golden_dataset(root, vec):
    """-> (db, sample dirs in the vectors' order)."""
    db = os.path.join(root, 'db')
    os.makedirs(db, exist_ok=True)
    with open(os.path.join(db, 'species_info.txt'), 'w') as h:
        h.write('species_id\trep_genome\tcount_genomes\n')
        for sp in vec['species']:
            h.write('%s\t%s.rep\t3\n' % (sp['id'], sp['id']))
    with open(os.path.join(db, 'genome_info.txt'), 'w') as h:
        h.write('genome_id\tspecies_id\n')
        for sp in vec['species']:
            h.write('%s.rep\t%s\n' % (sp['id'], sp['id']))
    dirs = []
    for sp in vec['species']:
        d = os.path.join(db, 'pan_genomes', sp['id'])
        os.makedirs(d, exist_ok=True)
        if sp['gene_info_gz']:
            with gzip.open(os.path.join(d, 'gene_info.txt.gz'), 'wb') as h:
                h.write(sp['gene_info'].encode())
            with open(os.path.join(d, 'gene_info.txt'), 'w') as h:
                h.write('centroid_99\tcentroid_95\n')
        else:
            with open(os.path.join(d, 'gene_info.txt'), 'w') as h:
                h.write(sp['gene_info'])
        for smp in sp['samples']:
            sd = os.path.join(root, 'samples', smp['id'])
            os.makedirs(os.path.join(sd, 'genes', 'output'), exist_ok=True)
            with gzip.open(os.path.join(sd, 'genes', 'output', '%s.genes.gz' % sp['id']), 'wb') as h:
                h.write(base64.b64decode(smp['table']))
            with open(os.path.join(sd, 'genes', 'summary.txt'), 'w') as h:
                h.write('\t'.join(('species_id',) + SUMMARY_FIELDS) + '\n')
                h.write('\t'.join([sp['id']] + [smp['summary'][f] for f in SUMMARY_FIELDS]) + '\n')
            dirs.append(sd)
    return db, dirs


def check_outputs(outdir, vec, pid):
    for sp in vec['species']:
        exp = sp['expected'][pid]
        for name in MATRICES + ('summary',):
            got = open(os.path.join(outdir, sp['id'], 'genes_%s.txt' % name)).read()
            assert got == exp[name], (sp['id'], pid, name)
        assert os.path.isfile(os.path.join(outdir, sp['id'], 'readme.txt'))
