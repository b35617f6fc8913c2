"""snp_diversity.py / call_consensus.py end to end on a seeded species directory, phase by phase.

Writes a directory in the shape of `merge_midas.py snps` output (default 2 000 000 sites x 50 samples, the size of BASELINE
configs[4]; '{:.3g}' frequencies) on tmpfs, then runs every mode as the commands do and prints where the time goes: reading the
tables (summary + info parsed, matrices mapped), the device call split into upload + index, index, parse, site kernel, order,
ordered sums, sequences and download, and writing the output.  The parser's rate is the bytes of both matrices over the parse
kernels' time, printed beside the device's own read-stream rate (measure.hip) taken in the same process.

usage: python tools/analyze_e2e.py [--sites 2000000] [--samples 50] [--genes 3000] [--dir /dev/shm] [--keep] [--out FILE]
"""
import argparse
import os
import shutil
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from midas_amd import abi  # noqa: E402
from midas_amd.analyze import cli, consensus, diversity, sites, synth  # noqa: E402

PHASES = ['upload+index', 'index', 'parse', 'site', 'order', 'sums', 'seq', 'download']
MODES = [
    ('per-sample genome-wide', 'snp_diversity.py', []),
    ('per-sample per-gene', 'snp_diversity.py', ['--genomic_type', 'per-gene', '--locus_type', 'CDS']),
    ('pooled genome-wide', 'snp_diversity.py', ['--sample_type', 'pooled-samples']),
    ('pooled per-gene weighted', 'snp_diversity.py', ['--sample_type', 'pooled-samples', '--genomic_type', 'per-gene', '--locus_type', 'CDS',
                                                      '--weight_by_depth']),
    ('call_consensus', 'call_consensus.py', ['--site_prev', '0.5']),
]


class Shared:
    def __init__(self, ctx):
        self._ctx = ctx

    def sites_scan(self, *a, **kw):
        return self._ctx.sites_scan(*a, **kw)

    def close(self):
        pass


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sites', type=int, default=2000000)
    ap.add_argument('--samples', type=int, default=50)
    ap.add_argument('--genes', type=int, default=3000)
    ap.add_argument('--dir', default='/dev/shm')
    ap.add_argument('--keep', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    root = tempfile.mkdtemp(prefix='analyze_e2e_', dir=a.dir)
    try:
        d = os.path.join(root, 'species_1')
        t0 = time.perf_counter()
        synth.write_species_dir(d, a.sites, a.samples, seed=4, n_genes=a.genes)
        nbytes = os.path.getsize(d + '/snps_freq.txt') + os.path.getsize(d + '/snps_depth.txt')
        say("inputs: %d sites x %d samples written in %.1f s; snps_freq.txt %.1f MB, snps_depth.txt %.1f MB"
            % (a.sites, a.samples, time.perf_counter() - t0, os.path.getsize(d + '/snps_freq.txt') / 1e6, os.path.getsize(d + '/snps_depth.txt') / 1e6))
        with abi.Context(0) as ctx:
            rates = ctx.stream_rates(1 << 30, 5)
            say("device read stream (measure.hip, same process): %.0f GB/s" % rates['read_GBps'])
            for k, (name, script, opts) in enumerate([MODES[0]] + MODES):       # (the first mode once more in front: warm-up)
                out = os.path.join(root, 'out.txt')
                parse, pipeline = (cli.diversity_arguments, diversity) if script == 'snp_diversity.py' else (cli.consensus_arguments, consensus)
                args = parse([d, '--out', out] + opts)
                t0 = time.perf_counter()
                tables = sites.open_tables(d)
                samples = sites.fetch_samples(tables, args['sample_depth'], args['fract_cov'], args['max_samples'])
                t1 = time.perf_counter()
                res = pipeline.compute(args, tables, samples, Shared(ctx))
                t2 = time.perf_counter()
                if script == 'snp_diversity.py':
                    diversity.write_pi(args, tables, samples, res)
                else:
                    consensus.write_consensus(args, samples, res['seq'])
                t3 = time.perf_counter()
                if k == 0:
                    continue
                say("%s: %d sites read, %d kept, %d group(s), cells converted by the host: %d" % (name, res['n_sites'], res['n_kept'], res['groups'],
                                                                                                 res['side_freq'] + res['side_depth']))
                say("  read tables  %8.3f s   device call (with host mask) %8.3f s   write %8.3f s   total %8.3f s" % (t1 - t0, t2 - t1, t3 - t2, t3 - t0))
                say("  " + "  ".join("%s %.2f ms" % (p, m) for p, m in zip(PHASES, res['ms'])))
                parse_ms = res['ms'][2]
                if parse_ms > 0:
                    gbps = nbytes / parse_ms / 1e6
                    say("  parser: %.1f MB of text in %.2f ms = %.1f GB/s (%.1f %% of the read stream); ordered sums %.2f ms, site kernel %.2f ms"
                        % (nbytes / 1e6, parse_ms, gbps, 100.0 * gbps / rates['read_GBps'], res['ms'][5], res['ms'][3]))
    finally:
        if not a.keep:
            shutil.rmtree(root, ignore_errors=True)
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
