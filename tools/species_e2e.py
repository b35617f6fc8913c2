#!/usr/bin/env python
"""run_species.py's classify step, timed by phase on one MI355X: 2 M synthetic m8 lines of 500 k reads against 5 952 species x 15
marker families (the size of the MIDAS database's marker set).

Phases (medians of nine runs after a warm-up): upload, line index, fields, lookup, filter + sort + group, best hits, download
(the library's own host clock around each, midas_species_classify's out_ms8), the serial chain on the host
(midas_species_assign) and the table.  Beside them, once: the same file through a per-line classify on the host -- the
reference's own functions when a MIDAS checkout is importable (MIDAS_REFERENCE=/path/to/MIDAS, with Biopython or without: a
stand-in for Bio.SeqIO.parse is supplied), else the sequential model of the tests.

usage: python tools/species_e2e.py [--lines N] [--runs K] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from midas_amd import abi  # noqa: E402
from midas_amd.run import species as mspecies  # noqa: E402


def make_input(n_lines, n_queries, n_species, n_markers, seed):
    """(model Database, MarkerDatabase-like arrays, text).  Vectorised: the text is built column by column."""
    from tests import species_model as M
    rng = np.random.default_rng(seed)
    species = ['S%05d' % k for k in range(n_species)]
    markers = ['B%06d' % (k + 1) for k in range(n_markers)]
    names = ['%d.%d.peg.%d' % (100000 + k, 1 + k % 3, 5 + 3 * m) for k in range(n_species) for m in range(n_markers)]
    lengths = rng.integers(300, 2000, size=len(names))
    genes = dict((g, (species[i // n_markers], markers[i % n_markers], int(lengths[i]))) for i, g in enumerate(names))
    cutoffs = dict((marker, 94.0 + 0.25 * (m % 16)) for m, marker in enumerate(markers))
    q = np.sort(rng.integers(0, n_queries, size=n_lines))
    qlen = np.array([75, 100, 150, 250])[q % 4]
    hot = rng.integers(0, n_species, size=200)
    sp = np.where(rng.random(n_lines) < 0.8, hot[rng.integers(0, 200, size=n_lines)], rng.integers(0, n_species, size=n_lines))
    gene = sp * n_markers + (q % n_markers)
    pid = rng.choice([93.0, 95.0, 96.5, 98.25, 99.0, 100.0], size=n_lines) + rng.integers(0, 100, size=n_lines) / 100
    aln = (qlen * rng.choice([0.5, 0.74, 0.75, 0.9, 1.0], size=n_lines)).astype(int)
    score = np.array([90.5, 120.0, 150.0, 187.0])[q % 4] - np.where(rng.random(n_lines) < 0.7, 0, rng.integers(1, 40, size=n_lines) / 2)
    lines = ['r%d_%d\t%s\t%.2f\t%d\t2\t0\t1\t%d\t11\t%d\t3e-40\t%s' % (a, b, names[c], d, e, e, 10 + e, f)
             for a, b, c, d, e, f in zip(q.tolist(), qlen.tolist(), gene.tolist(), pid.tolist(), aln.tolist(), score.tolist())]
    return M.Database(species, genes, cutoffs), '\n'.join(lines) + '\n'


class Arrays:
    def __init__(self, db):
        sp = dict((s, k) for k, s in enumerate(db.species))
        self.species = db.species
        self.markers = sorted(db.cutoffs)
        mk = dict((m, k) for k, m in enumerate(self.markers))
        self.gene_names = [g.encode() for g in db.genes]
        self.gene_species = np.array([sp[v[0]] for v in db.genes.values()], np.int32)
        self.gene_marker = np.array([mk[v[1]] for v in db.genes.values()], np.int32)
        self.cutoff = np.array([db.cutoffs[m] for m in self.markers])
        self.marker_length = [0] * len(db.species)
        for v in db.genes.values():
            self.marker_length[sp[v[0]]] += v[2]


def host_classify(db, text, tmp):
    """The per-line classify on this box's host, once -> (seconds, what ran)."""
    from tests import species_model as M
    ref = os.environ.get('MIDAS_REFERENCE')
    if ref and os.path.isdir(os.path.join(ref, 'midas')):
        sys.path.insert(0, ref)
        try:
            import Bio.SeqIO  # noqa: F401
        except ImportError:
            import types
            bio, seqio = types.ModuleType('Bio'), types.ModuleType('Bio.SeqIO')

            def parse(path, fmt):
                for line in open(path):
                    if line.startswith('>'):
                        yield types.SimpleNamespace(id=line[1:].split()[0])
            seqio.parse = parse
            bio.SeqIO = seqio
            sys.modules['Bio'], sys.modules['Bio.SeqIO'] = bio, seqio
        from midas.run import species as S
        files = dict(species_info='species_id\n' + ''.join(s + '\n' for s in db.species),
                     phyeco_fa=''.join('>%s\nACGT\n' % g for g in db.genes),
                     phyeco_map='species_id\tgene_id\tgene_length\tmarker_id\n' + ''.join('%s\t%s\t%d\t%s\n' % (v[0], g, v[2], v[1]) for g, v in db.genes.items()),
                     phyeco_mapping_cutoffs=''.join('%s\t%s\n' % kv for kv in db.cutoffs.items()))
        M.write_db(os.path.join(tmp, 'db'), files)
        out = M.write_sample(os.path.join(tmp, 'sample'), text)
        args = dict(db=os.path.join(tmp, 'db'), outdir=out, mapid=None, aln_cov=0.75)
        info, markers = S.read_annotations(args), S.read_marker_info(args)
        t0 = time.time()
        best = S.find_best_hits(args, markers)
        alns = S.assign_non_unique(args, best, S.assign_unique(args, best, info, markers), markers)
        S.normalize_counts(alns, S.read_gene_lengths(args, info, markers))
        return time.time() - t0, "the reference's find_best_hits .. normalize_counts"
    t0 = time.time()
    M.classify(text, db, seed=1)
    return time.time() - t0, "the tests' sequential model (no MIDAS checkout at $MIDAS_REFERENCE)"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--lines', type=int, default=2000000)
    ap.add_argument('--queries', type=int, default=500000)
    ap.add_argument('--species', type=int, default=5952)
    ap.add_argument('--markers', type=int, default=15)
    ap.add_argument('--runs', type=int, default=9)
    ap.add_argument('--out')
    ap.add_argument('--no_host', action='store_true')
    a = ap.parse_args()
    import random
    import tempfile
    db, text = make_input(a.lines, a.queries, a.species, a.markers, 1)
    arr = Arrays(db)
    raw = np.frombuffer(text.encode(), np.uint8)
    random.seed(1)
    np.random.seed(1)
    py_state, np_state = random.getstate(), np.random.get_state()
    rows = []
    with abi.Context(0) as ctx:
        for run in range(a.runs + 1):          # the first one warms up (code objects, the allocator)
            t0 = time.time()
            reads, bases, hits = mspecies.classify(ctx, raw, arr, 0.75, py_state=py_state, np_state=np_state)
            t1 = time.time()
            table, total = mspecies.abundance(arr, reads, bases)
            t2 = time.time()
            if run:
                rows.append(hits['ms'][:7] + [hits['chain_ms'], (t2 - t1) * 1e3, (t2 - t0) * 1e3])
    names = list(abi.SPECIES_PHASES) + ['host chain', 'table', 'classify + chain + table, wall']
    med = [statistics.median(r[k] for r in rows) for k in range(len(names))]
    out = ["species_e2e.py: %d lines, %d bytes, %d reads, %d species x %d marker families; %d passing lines, %d unique and %d ambiguous reads, "
           "%d cells parsed by the host" % (hits['lines'], raw.size, a.queries, a.species, a.markers, hits['passing'], hits['unique'], hits['ambiguous'],
                                          hits['side_cells']),
           "medians of %d runs after one warm-up, ms (min .. max)" % a.runs]
    for k, n in enumerate(names):
        out.append("  %-34s %10.2f   (%.2f .. %.2f)" % (n, med[k], min(r[k] for r in rows), max(r[k] for r in rows)))
    out.append("  total marker-gene coverage %s; most abundant: %s" % (round(total, 3), table[0][:2]))
    if not a.no_host:
        with tempfile.TemporaryDirectory() as tmp:
            sec, what = host_classify(db, text, tmp)
        out.append("host, one run: %.1f s -- %s" % (sec, what))
        out.append("  ratio to the wall median above: %.0fx" % (sec * 1e3 / med[-1]))
    print('\n'.join(out))
    if a.out:
        with open(a.out, 'w') as handle:
            handle.write('\n'.join(out) + '\n')


if __name__ == '__main__':
    main()
