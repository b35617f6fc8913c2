#!/usr/bin/env python
"""Phases of merge_species.py on a synthetic input of the default database's size: 5 952 species x 2 000 samples, seeded, every
species in every profile, rows shuffled per sample.  Prints (and with --out writes, e.g. profiles/merge_species.txt) the medians of
the phases -- read (the time the device waits for the host's readers), upload, index, fields, lookup + scatter, statistics,
download, write -- and beside them the wall time of the tests' sequential model (np.mean / np.median / str per species, as
midas/merge/species.py does it) on the first --model_samples samples of the same input.

usage: python tools/merge_species_e2e.py [--species 5952] [--samples 2000] [--runs 5] [--model_samples 100] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from midas_amd import abi  # noqa: E402
from tests import merge_species_model as M  # noqa: E402


def make_input(root, n_species, n_samples, seed):
    """Profiles as run_species.py writes them: repr doubles, one row a species.  -> (species ids, sample ids, paths, bytes)."""
    rng = np.random.default_rng(seed)
    ids = ['Species_name_%05d' % k for k in range(n_species)]
    sample_ids = ['sample_%05d' % s for s in range(n_samples)]
    paths, total = [], 0
    for s in sample_ids:
        reads = rng.integers(0, 5000, n_species) * (rng.random(n_species) < 0.2)
        cov = reads * rng.random(n_species) * 0.05
        ab = cov / max(cov.sum(), 1e-300)
        order = rng.permutation(n_species)
        text = 'species_id\tcount_reads\tcoverage\trelative_abundance\n' + ''.join(
            '%s\t%d\t%s\t%s\n' % (ids[k], reads[k], repr(float(cov[k])), repr(float(ab[k]))) for k in order)
        os.makedirs(os.path.join(root, s, 'species'))
        paths.append(os.path.join(root, s, 'species', 'species_profile.txt'))
        with open(paths[-1], 'w') as handle:
            handle.write(text)
        total += len(text)
    return ids, sample_ids, paths, total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--species', type=int, default=5952)
    ap.add_argument('--samples', type=int, default=2000)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--model_samples', type=int, default=100)
    ap.add_argument('--chunk_bytes', type=int, default=0)
    ap.add_argument('--out')
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        ids, sample_ids, paths, total = make_input(os.path.join(tmp, 'in'), a.species, a.samples, 1)
        rows = []
        with abi.Context(0) as ctx:
            for run in range(a.runs + 1):          # the first one warms up (code objects, the allocator, the page cache)
                out = os.path.join(tmp, 'out_%d' % run)
                os.makedirs(out)
                t0 = time.time()
                with ctx.species_merge(paths, ids, 1.0, chunk_bytes=a.chunk_bytes) as res:
                    t1 = time.time()
                    res.write(out, sample_ids)
                    t2 = time.time()
                    if run:
                        rows.append(res.ms[:7] + [(t2 - t1) * 1e3, (t2 - t0) * 1e3])
                    facts = (res.lines, res.groups, res.chunk_bytes, res.side_cells, res.lds_rows)
        names = list(abi.SPECIES_MERGE_PHASES) + ['write', 'merge + write, wall']
        med = [statistics.median(r[k] for r in rows) for k in range(len(names))]
        lines = ["merge_species_e2e.py: %d species x %d samples, %d bytes of profiles, %d lines in %d groups of at most %d bytes, %d cells parsed by "
                 "the host, rows sorted in %s" % (a.species, a.samples, total, facts[0], facts[1], facts[2], facts[3], 'LDS' if facts[4] else 'the radix sort'),
                 "medians of %d runs after one warm-up, ms (min .. max)" % a.runs]
        for k, n in enumerate(names):
            lines.append("  %-22s %10.2f   (%.2f .. %.2f)" % (n, med[k], min(r[k] for r in rows), max(r[k] for r in rows)))
        n = min(a.model_samples, a.samples)
        if n > 0:
            texts = [open(q).read() for q in paths[:n]]
            t0 = time.time()
            got = M.merge(sample_ids[:n], texts, ids, 1.0)
            sec = time.time() - t0
            lines.append("the tests' sequential model on the first %d samples, one run: %.1f s (%.1f ms a sample; x %d samples = %.0f s)"
                         % (n, sec, sec * 1e3 / n, a.samples, sec / n * a.samples))
            with abi.Context(0) as ctx, ctx.species_merge(paths[:n], ids, 1.0) as res:
                same = all(np.array_equal(np.asarray(got[k], np.float64).view(np.uint64), getattr(res, k).view(np.uint64)) for k in abi.SPECIES_MERGE_STATS)
                same = same and res.order.tolist() == got['order'] and np.array_equal(res.coverage, np.asarray(got['coverage']))
            lines.append("  the device's result on those samples equals the model's: %s" % same)
    print('\n'.join(lines))
    if a.out:
        with open(a.out, 'w') as handle:
            handle.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
