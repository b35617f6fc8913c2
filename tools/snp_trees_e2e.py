"""snp_trees.py end to end on a seeded species directory, phase by phase.

Writes a directory in the shape of `merge_midas.py snps` output on tmpfs (midas_amd/analyze/synth.py write_species_dir), then
does what the command does -- tables, sample selection, site mask, Context.sites_consensus_pairs, the division,
Context.nj_tree, the Newick text and the pair table -- several times, and prints the median of every phase: upload + index
(host clock around the copies), index, parse, site kernel, planes, pairs (device events of the first call), NJ (device events
around all of its steps), write (host clock: both files).  The first pass is a warm-up and is left out.

Two cases by default: 2 000 000 sites x 50 samples, and a wide one of 100 000 sites x 1 000 samples.

usage: python tools/snp_trees_e2e.py [--cases 2000000x50,100000x1000] [--reps 5] [--dir /dev/shm] [--keep] [--out FILE]
"""
import argparse
import os
import shutil
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from midas_amd import abi  # noqa: E402
from midas_amd.analyze import cli, sites, synth, trees  # noqa: E402

PHASES = ['upload+index', 'index', 'parse', 'site', 'planes', 'pairs', 'NJ', 'write']


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='2000000x50,100000x1000')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--dir', default='/dev/shm')
    ap.add_argument('--keep', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    root = tempfile.mkdtemp(prefix='snp_trees_e2e_', dir=a.dir)
    try:
        with abi.Context(0) as ctx:
            say("device: %s" % ctx.device_info()['name'])
            for case in a.cases.split(','):
                n_sites, n_samples = (int(x) for x in case.split('x'))
                d = os.path.join(root, 'species_%s' % case)
                t0 = time.perf_counter()
                synth.write_species_dir(d, n_sites, n_samples, seed=4, block=max(1000, 4000000 // n_samples))
                say("inputs: %d sites x %d samples written in %.1f s; snps_freq.txt %.1f MB, snps_depth.txt %.1f MB"
                    % (n_sites, n_samples, time.perf_counter() - t0, os.path.getsize(d + '/snps_freq.txt') / 1e6,
                       os.path.getsize(d + '/snps_depth.txt') / 1e6))
                nwk, pairs = os.path.join(root, 'tree.nwk'), os.path.join(root, 'pairs.txt')
                args = cli.trees_arguments([d, '--out', nwk, '--dist', pairs])
                runs, calls = [], []
                for k in range(a.reps + 1):
                    t0 = time.perf_counter()
                    tables = sites.open_tables(d)
                    samples = sites.fetch_samples(tables, args['sample_depth'], args['fract_cov'], args['max_samples'])
                    cli.check_tree_samples(list(samples))
                    t1 = time.perf_counter()
                    res = trees.compute(args, tables, samples, ctx)
                    t2 = time.perf_counter()
                    names = list(samples)
                    with open(nwk, 'w') as out:
                        out.write(trees.newick(names, res['tree']))
                    trees.write_pairs(pairs, names, res['both'], res['diff'], res['dist'])
                    t3 = time.perf_counter()
                    if k == 0:
                        continue                                                     # (the first pass: warm-up)
                    ms = res['ms']
                    runs.append([ms[0], ms[1], ms[2], ms[3], ms[4], ms[5], res['tree']['ms'][1], (t3 - t2) * 1e3])
                    calls.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3, t3 - t0))
                med = [statistics.median(r[k] for r in runs) for k in range(len(PHASES))]
                say("snp_trees.py: %d sites read, %d retained, %d group(s), %d pairs of samples, cells converted by the host: %d"
                    % (res['n_sites'], res['n_kept'], res['groups'], n_samples * (n_samples - 1) // 2, res['side_freq'] + res['side_depth']))
                say("  medians of %d runs:  " % a.reps + "  ".join("%s %.2f ms" % (p, m) for p, m in zip(PHASES, med)))
                say("  read tables %.1f ms   device calls + division %.1f ms   whole command %.3f s (medians)"
                    % (statistics.median(c[0] for c in calls), statistics.median(c[1] for c in calls), statistics.median(c[2] for c in calls)))
                say("  pair kernel: %d word-pairs (S(S+1)/2 x words, two planes each) = %.0f G word-pairs/s; at most %d runs of at most %d staging steps"
                    % (res['word_pairs'], res['word_pairs'] / max(med[5], 1e-9) / 1e6, res['pair_runs'], res['pair_steps']))
                say("  NJ: %d steps, %d launches, %.1f us a step; files: tree %.2f MB, pairs %.2f MB"
                    % (n_samples - 3, 4 * (n_samples - 3) + 1, med[6] * 1e3 / max(n_samples - 3, 1), os.path.getsize(nwk) / 1e6,
                       os.path.getsize(pairs) / 1e6))
                assert np.isfinite(res['dist']).all()
                if not a.keep:
                    shutil.rmtree(d, ignore_errors=True)
    finally:
        if not a.keep:
            shutil.rmtree(root, ignore_errors=True)
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
