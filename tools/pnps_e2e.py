"""snp_pnps.py's one device pass against the two snp_diversity.py device calls it replaces, on a seeded species directory.

Writes a directory in the shape of `merge_midas.py snps` output (default 2 000 000 sites x 50 samples, 3000 genes, as
tools/analyze_e2e.py) on tmpfs and, for the four modes (per-sample and pooled, each genome-wide and per-gene), runs in one
process, the three calls taking turns, after one warm-up round, 7 rounds:

  pnps   Context.sites_scan_classes over the CDS 1D + 4D sites, two classes (the classed sums kernel)
  1D     Context.sites_scan over the CDS 1D sites (the existing sums kernel)
  4D     Context.sites_scan over the CDS 4D sites

The host masks are made once, outside the clock; a time is the wall clock around the device call, the phases are the call's own
out_ms8.  Before any time is printed the two blocks of the one pass are held against the two calls: pi by bits, the integers
exactly.  The bar: the one pass's median is below the sum of the two calls' medians by more than the larger of the two
spreads (max - min over the rounds of the one pass, and of the round-by-round sums of the two calls).

usage: python tools/pnps_e2e.py [--sites 2000000] [--samples 50] [--genes 3000] [--rounds 7] [--dir /dev/shm] [--keep] [--out FILE]
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
from midas_amd.analyze import cli, diversity, pnps, sites, synth  # noqa: E402

PHASES = ['upload+index', 'index', 'parse', 'site', 'order', 'sums', 'seq', 'download']
MODES = [
    ('per-sample genome-wide', []),
    ('per-sample per-gene', ['--genomic_type', 'per-gene']),
    ('pooled genome-wide', ['--sample_type', 'pooled-samples']),
    ('pooled per-gene', ['--sample_type', 'pooled-samples', '--genomic_type', 'per-gene']),
]


def flags_of(args):
    return abi.SITES_SUMS | (abi.SITES_POOLED if args['sample_type'] == 'pooled-samples' else 0) | \
        (abi.SITES_PER_GENE if args['genomic_type'] == 'per-gene' else 0)


def spread(v):
    return "%.1f [%.1f .. %.1f]" % (statistics.median(v), min(v), max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sites', type=int, default=2000000)
    ap.add_argument('--samples', type=int, default=50)
    ap.add_argument('--genes', type=int, default=3000)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--dir', default='/dev/shm')
    ap.add_argument('--keep', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    root = tempfile.mkdtemp(prefix='pnps_e2e_', dir=a.dir)
    try:
        d = os.path.join(root, 'species_1')
        t0 = time.perf_counter()
        synth.write_species_dir(d, a.sites, a.samples, seed=4, n_genes=a.genes)
        say("inputs: %d sites x %d samples, %d genes written in %.1f s; snps_freq.txt %.1f MB, snps_depth.txt %.1f MB"
            % (a.sites, a.samples, a.genes, time.perf_counter() - t0, os.path.getsize(d + '/snps_freq.txt') / 1e6,
               os.path.getsize(d + '/snps_depth.txt') / 1e6))
        tables = sites.open_tables(d)
        verdicts = []
        with abi.Context(0) as ctx:
            for name, opts in MODES:
                args = cli.pnps_arguments([d] + opts)
                samples = sites.fetch_samples(tables, args['sample_depth'], args['fract_cov'], args['max_samples'])
                flags = flags_of(args)
                per_gene = bool(flags & abi.SITES_PER_GENE)
                mask, site_class, n = pnps.class_mask(tables, args)
                common = dict(snp_maf=float(args['snp_maf']), site_gene=tables.gene[:n] if per_gene else None, n_genes=tables.n_genes)
                calls = [('pnps', lambda: sites.scan(ctx, tables, samples, mask, n, args, flags, classes=(site_class, len(pnps.CLASSES)), **common))]
                for c, cname in enumerate(pnps.CLASSES):
                    one, n1 = diversity.site_mask(tables, dict(args, locus_type='CDS', site_type=cname, site_list=None, rand_sites=None))
                    assert n1 == n and np.array_equal(one, mask & (site_class == c))
                    calls.append((cname, lambda one=one: sites.scan(ctx, tables, samples, one, n, args, flags, **common)))
                wall = {k: [] for k, _ in calls}
                sums = {k: [] for k, _ in calls}
                phases = {}
                for r in range(a.rounds + 1):                                         # (round 0: warm-up)
                    res = {}
                    for k, call in calls:
                        t0 = time.perf_counter()
                        res[k] = call()
                        t = (time.perf_counter() - t0) * 1e3
                        if r:
                            wall[k].append(t)
                            sums[k].append(res[k]['ms'][5])
                            phases.setdefault(k, []).append(res[k]['ms'])
                    for c, cname in enumerate(pnps.CLASSES):                         # the numbers agree, or no time is printed
                        for q in ('snps', 'sites', 'depth'):
                            assert np.array_equal(res['pnps'][q][c], res[cname][q]), (name, cname, q)
                        assert np.array_equal(res['pnps']['pi'][c].view(np.uint64), res[cname]['pi'].view(np.uint64)), (name, cname, 'pi')
                    assert res['pnps']['n_kept'] == res['1D']['n_kept'] + res['4D']['n_kept']
                both = [x + y for x, y in zip(wall['1D'], wall['4D'])]
                both_sums = [x + y for x, y in zip(sums['1D'], sums['4D'])]
                gain = statistics.median(wall['1D']) + statistics.median(wall['4D']) - statistics.median(wall['pnps'])
                bar = max(max(wall['pnps']) - min(wall['pnps']), max(both) - min(both))
                met = gain > bar
                verdicts.append(met)
                say("%s: %d sites read, %d kept (1D %d, 4D %d), %d group(s); blocks equal to the two calls bit for bit"
                    % (name, res['pnps']['n_sites'], res['pnps']['n_kept'], res['1D']['n_kept'], res['4D']['n_kept'], res['pnps']['groups']))
                say("  device call ms, median [min .. max] of %d:  pnps %s   1D %s   4D %s   1D + 4D by round %s"
                    % (a.rounds, spread(wall['pnps']), spread(wall['1D']), spread(wall['4D']), spread(both)))
                say("  sums phase ms:  classed kernel (both classes, one launch a group) %s   existing kernel 1D %s   4D %s   1D + 4D %s"
                    % (spread(sums['pnps']), spread(sums['1D']), spread(sums['4D']), spread(both_sums)))
                for k, _ in calls:
                    med = [statistics.median(p[i] for p in phases[k]) for i in range(8)]
                    say("  %-4s phases (medians): " % k + "  ".join("%s %.2f" % (p, m) for p, m in zip(PHASES, med)))
                say("  bar: median(1D) + median(4D) - median(pnps) = %.1f ms against the larger spread %.1f ms: %s"
                    % (gain, bar, "MET" if met else "NOT MET"))
        say("verdict: the bar is %s (%d of %d modes)" % ("MET" if all(verdicts) else "NOT MET", sum(verdicts), len(verdicts)))
    finally:
        if not a.keep:
            shutil.rmtree(root, ignore_errors=True)
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
