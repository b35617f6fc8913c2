"""snp_pairs.py's one device pass against the separate two-sample pooled calls it replaces, on seeded species directories.

Writes a directory in the shape of `merge_midas.py snps` output on tmpfs, by default at both shapes in turn: 2 000 000 sites x
50 samples (few pairs behind a long site axis) and 100 000 sites x 1 000 samples (half a million pairs).  Per shape, in one process:

  check   Context.sites_pair_diversity against Context.sites_scan (SITES_SUMS | SITES_POOLED over the two columns) on a handful
          of pairs: pi by bits, sites and snps exactly.  No time is printed before this holds.
  forms   the one pass with either kernel form forced (pair_form 1: one pair a lane, tiles of 16 x 16; pair_form 2: a 4 x 4 patch a
          lane, tiles of 64 x 64), one warm-up and --rounds rounds each: the wall clock around the call, the call's own phases,
          and the pair kernel's pair-sites per second.  Both forms must give the same bits.
  today   one separate two-sample call on the same commit, median of the rounds, multiplied by the number of pairs: what a user
          pays today, without the process start and the file reads of each run.

usage: python tools/snp_pairs_e2e.py [--shapes 2000000x50,100000x1000] [--rounds 3] [--dir /dev/shm] [--keep] [--out FILE]
"""
import argparse
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from midas_amd import abi  # noqa: E402
from midas_amd.analyze import cli, diversity, sites, synth  # noqa: E402

PHASES = ['upload+index', 'index', 'parse', 'site', 'order', 'pairs', '-', 'download']
FORMS = ((1, 'one pair a lane, 16 x 16 tiles'), (2, '4 x 4 patch a lane, 64 x 64 tiles'))


def spread(v):
    return "%.1f [%.1f .. %.1f]" % (statistics.median(v), min(v), max(v))


def one_shape(ctx, say, root, n_sites, n_samples, rounds):
    d = os.path.join(root, 'species_%dx%d' % (n_sites, n_samples))
    t0 = time.perf_counter()
    synth.write_species_dir(d, n_sites, n_samples, seed=4)
    say("inputs: %d sites x %d samples written in %.1f s; snps_freq.txt %.1f MB, snps_depth.txt %.1f MB"
        % (n_sites, n_samples, time.perf_counter() - t0, os.path.getsize(d + '/snps_freq.txt') / 1e6, os.path.getsize(d + '/snps_depth.txt') / 1e6))
    tables = sites.open_tables(d)
    args = cli.pairs_arguments([d])
    samples = sites.fetch_samples(tables, args['sample_depth'], args['fract_cov'], args['max_samples'])
    order = list(samples.values())
    mask, n = diversity.site_mask(tables, args)
    mask = np.ascontiguousarray(mask[:n], np.uint8)
    cols, mean = [s.index for s in order], [s.mean_depth for s in order]
    common = (int(args['site_depth']), float(args['site_ratio']), float(args['allele_support']), float(args['site_prev']), float(args['site_maf']))
    S = len(order)
    n_pairs = S * (S - 1) // 2

    def pass_(form):
        return ctx.sites_pair_diversity(tables.freq_text, tables.depth_text, mask, cols, mean, *common, snp_maf=float(args['snp_maf']), pair_form=form)

    def two(i, j):
        return ctx.sites_scan(tables.freq_text, tables.depth_text, mask, [cols[i], cols[j]], [mean[i], mean[j]], *common,
                              snp_maf=float(args['snp_maf']), flags=abi.SITES_SUMS | abi.SITES_POOLED)

    first = pass_(0)
    picks = sorted({(0, 1), (0, S - 1), (S // 2, S // 2 + 1), (S - 2, S - 1), (1, S // 3 + 2)})
    for i, j in picks:
        one = two(i, j)
        assert first['sites'][i, j] == one['sites'][0, 0] and first['snps'][i, j] == one['snps'][0, 0], (i, j)
        assert first['pi'][i, j].view(np.uint64) == one['pi'][0, 0].view(np.uint64), (i, j)
    say("check: %d pairs equal the separate pooled calls, pi bit for bit; %d pairs, %d sites read, %d group(s); default form: %d pair(s) a lane a side, %d tiles"
        % (len(picks), n_pairs, first['n_sites'], first['groups'], first['pair_form'], first['tiles']))
    results = {}
    for form, name in FORMS:
        wall, phases = [], []
        for r in range(rounds + 1):                                  # (round 0: warm-up)
            t0 = time.perf_counter()
            res = pass_(form)
            t = (time.perf_counter() - t0) * 1e3
            if r:
                wall.append(t)
                phases.append(res['ms'])
        for k in ('sites', 'snps', 'shared'):
            assert np.array_equal(res[k], first[k]), (form, k)
        for k in ('pi', 'w1', 'w2', 'x'):
            assert np.array_equal(res[k].view(np.uint64), first[k].view(np.uint64)), (form, k)
        med = [statistics.median(p[i] for p in phases) for i in range(8)]
        results[form] = (statistics.median(wall), med[5])
        say("form %d (%s), %d tiles: device call ms %s" % (form, name, res['tiles'], spread(wall)))
        say("  phases (medians): " + "  ".join("%s %.2f" % (p, m) for p, m in zip(PHASES, med) if p != '-'))
        say("  pair kernel: %.3g pair-sites in %.1f ms = %.3g pair-sites/s" % (res['pair_sites'], med[5], res['pair_sites'] / (med[5] * 1e-3)))
    one_ms = []
    for r in range(rounds + 1):
        t0 = time.perf_counter()
        two(0, 1)
        if r:
            one_ms.append((time.perf_counter() - t0) * 1e3)
    best = min(results, key=lambda f: results[f][0])
    side64 = (S + 63) // 64
    say("today: one separate two-sample call ms %s; x %d pairs = %.1f s; the one pass (form %d) %.1f ms: %.0f x"
        % (spread(one_ms), n_pairs, statistics.median(one_ms) * n_pairs / 1e3, best, results[best][0], statistics.median(one_ms) * n_pairs / results[best][0]))
    say("forms: %d samples = %d tiles of 64 x 64: pair kernel ms form 1 %.1f, form 2 %.1f -> form %d is faster"
        % (S, side64 * (side64 + 1) // 2, results[1][1], results[2][1], 1 if results[1][1] <= results[2][1] else 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='2000000x50,100000x1000')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--dir', default='/dev/shm')
    ap.add_argument('--keep', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:
            with open(a.out, 'w') as f:
                f.write('\n'.join(lines) + '\n')

    root = tempfile.mkdtemp(prefix='snp_pairs_e2e_', dir=a.dir)
    try:
        with abi.Context(0) as ctx:
            for shape in a.shapes.split(','):
                n_sites, n_samples = (int(x) for x in shape.split('x'))
                one_shape(ctx, say, root, n_sites, n_samples, a.rounds)
                if not a.keep:
                    shutil.rmtree(os.path.join(root, 'species_%dx%d' % (n_sites, n_samples)), ignore_errors=True)
    finally:
        if not a.keep:
            shutil.rmtree(root, ignore_errors=True)


if __name__ == '__main__':
    main()
