"""snp_ld.py's device call on seeded species directories: its phases, pair-sites per second, and the sequential model beside it.

Writes a directory in the shape of `merge_midas.py snps` output on tmpfs, by default at both shapes in turn: 2 000 000 sites x
50 samples (one word of samples, a long site axis) and 100 000 sites x 1 000 samples (16 words).  The sites stand at consecutive
positions of one contig, so with --max_dist 1000 every anchor has up to 1 000 partners.  Per shape, in one process:

  check   Context.sites_ld over the first --slice rows against the sequential model (tests/snp_ld_model.py): the counts exactly,
          the three sums bit for bit.  No time is printed before this holds.  The model's own time over the slice is kept.
  call    the whole table, one warm-up and --rounds rounds: the wall clock around the call, the call's own phases, and the LD
          kernel's pair-sites per second (pairs of sites visited; each costs four popcounts a word of samples).
  model   the model's time over the slice, scaled by pairs to the whole table and MARKED AS SCALED: what the interpreted loop
          over pairs of sites would take on this host.

usage: python tools/snp_ld_e2e.py [--shapes 2000000x50,100000x1000] [--rounds 3] [--slice 1200] [--dir /dev/shm] [--keep] [--out FILE]
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
from midas_amd.analyze import cli, ld, sites, synth, trees  # noqa: E402
from tests import snp_ld_model  # noqa: E402

PHASES = ['upload+index', 'index', 'parse', 'site', 'planes', 'ld', 'fold', 'download']


def spread(v):
    return "%.1f [%.1f .. %.1f]" % (statistics.median(v), min(v), max(v))


def one_shape(ctx, say, root, n_sites, n_samples, rounds, n_slice):
    d = os.path.join(root, 'species_%dx%d' % (n_sites, n_samples))
    t0 = time.perf_counter()
    synth.write_species_dir(d, n_sites, n_samples, seed=4)
    say("inputs: %d sites x %d samples written in %.1f s; snps_freq.txt %.1f MB, snps_depth.txt %.1f MB"
        % (n_sites, n_samples, time.perf_counter() - t0, os.path.getsize(d + '/snps_freq.txt') / 1e6, os.path.getsize(d + '/snps_depth.txt') / 1e6))
    tables = sites.open_tables(d)
    args = cli.ld_arguments([d])
    order = list(sites.fetch_samples(tables, args['sample_depth'], args['fract_cov'], args['max_samples']).values())
    mask, flags = trees.site_mask(args, tables)
    mask = np.ascontiguousarray(mask, np.uint8)
    t0 = time.perf_counter()
    key = ld.site_keys(tables, mask)
    say("host: positions read, keys formed and their order checked in %.1f ms" % ((time.perf_counter() - t0) * 1e3))
    cols, mean = [s.index for s in order], [s.mean_depth for s in order]
    common = (int(args['site_depth']), float(args['site_ratio']), float(args['allele_support']), float(args['site_prev']), float(args['site_maf']))
    kw = dict(max_dist=args['max_dist'], bin_width=args['bin_width'], min_samples=args['min_samples'], flags=flags)

    def call(n):
        return ctx.sites_ld(tables.freq_text, tables.depth_text, mask[:n], cols, mean, key[:n], None, *common, **kw)

    n_slice = min(n_slice, n_sites)
    t0 = time.perf_counter()
    exp = snp_ld_model.sites_ld(tables.freq_text, tables.depth_text, mask[:n_slice], cols, mean, key[:n_slice], None, *common, **kw)
    model_s = time.perf_counter() - t0
    got = call(n_slice)
    assert np.array_equal(got['window'], exp['window']) and np.array_equal(got['pairs'], exp['pairs'])
    for k in ('sum_r2', 'sum_d2', 'sum_het'):
        assert got[k].tobytes() == exp[k].tobytes(), k
    say("check: the first %d rows equal the sequential model, sums bit for bit: %d sites retained, %d pairs of sites, %d informative; the model took %.2f s"
        % (n_slice, exp['n_kept'], exp['pairs_visited'], int(exp['pairs'].sum()), model_s))
    wall, phases = [], []
    for r in range(rounds + 1):                                      # (round 0: warm-up)
        t0 = time.perf_counter()
        res = call(n_sites)
        t = (time.perf_counter() - t0) * 1e3
        if r:
            wall.append(t)
            phases.append(res['ms'])
    med = [statistics.median(p[i] for p in phases) for i in range(8)]
    say("device call: %d sites read, %d retained, %d group(s), %d anchor chunk(s) of %d; ms %s"
        % (res['n_sites'], res['n_kept'], res['groups'], res['anchor_chunks'], res['anchor_chunk'], spread(wall)))
    say("  phases (medians): " + "  ".join("%s %.2f" % (p, m) for p, m in zip(PHASES, med)))
    say("  LD kernel: %.3g pairs of sites (%d informative) in %.1f ms = %.3g pair-sites/s; with the fold %.3g"
        % (res['pairs_visited'], int(res['pairs'].sum()), med[5], res['pairs_visited'] / (med[5] * 1e-3), res['pairs_visited'] / ((med[5] + med[6]) * 1e-3)))
    scaled = model_s * res['pairs_visited'] / max(exp['pairs_visited'], 1)
    say("model: %.2f s for %d pairs of sites on this host; SCALED by pairs to %d: %.0f s (%.1f h) -- %.0f x the device call"
        % (model_s, exp['pairs_visited'], res['pairs_visited'], scaled, scaled / 3600.0, scaled * 1e3 / statistics.median(wall)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='2000000x50,100000x1000')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--slice', type=int, default=1200)
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

    root = tempfile.mkdtemp(prefix='snp_ld_e2e_', dir=a.dir)
    try:
        with abi.Context(0) as ctx:
            for shape in a.shapes.split(','):
                n_sites, n_samples = (int(x) for x in shape.split('x'))
                one_shape(ctx, say, root, n_sites, n_samples, a.rounds, a.slice)
                if not a.keep:
                    shutil.rmtree(os.path.join(root, 'species_%dx%d' % (n_sites, n_samples)), ignore_errors=True)
    finally:
        if not a.keep:
            shutil.rmtree(root, ignore_errors=True)


if __name__ == '__main__':
    main()
