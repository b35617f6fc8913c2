"""strain_tracking.py end to end on a seeded species directory, phase by phase.

Writes a directory in the shape of `merge_midas.py snps` output on tmpfs (mostly fixed sites with planted private and shared
alleles: midas_amd/analyze/synth.py write_strain_species_dir), then runs id_markers and, on its output, track_markers as the
commands do, and prints where the time goes: reading the tables, the host's walk of the marker list, the device calls split
into upload + index, index, parse, allele call / matched sites, compaction / bit matrix, pairs and download, and the native
writers.  The pair kernel's rate is word-pairs per second -- (sample pairs with i <= j) x (64-site words of the bit matrices) --
printed beside the device's own read-stream rate (measure.hip) taken in the same process.  A pair launch lasts tens of
microseconds, so the device call of track_markers is repeated (--reps) and the pair phase given as median, least and most.

Two cases by default: 2 000 000 sites x 50 samples, and a wide one of 100 000 sites x 1 000 samples (the site count cut so that
the generator's arrays fit the host).

usage: python tools/strains_e2e.py [--cases 2000000x50,100000x1000] [--allele_prev 1] [--reps 9] [--dir /dev/shm] [--keep] [--out FILE]
"""
import argparse
import os
import shutil
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from midas_amd import abi  # noqa: E402
from midas_amd.analyze import sites, strains, synth  # noqa: E402

ID_PHASES = ['upload+index', 'index', 'parse', 'allele call', 'compact', '-', '-', 'download']
TRACK_PHASES = ['upload+index', 'index', 'parse', 'matched sites', 'bit matrix', 'pairs', '-', 'download']


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='2000000x50,100000x1000')
    ap.add_argument('--allele_prev', type=int, default=1)
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--dir', default='/dev/shm')
    ap.add_argument('--keep', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def phases(names, ms):
        return "  " + "  ".join("%s %.2f ms" % (p, m) for p, m in zip(names, ms) if p != '-')

    root = tempfile.mkdtemp(prefix='strains_e2e_', dir=a.dir)
    try:
        with abi.Context(0) as ctx:
            rates = ctx.stream_rates(1 << 30, 5)
            say("device read stream (measure.hip, same process): %.0f GB/s" % rates['read_GBps'])
            for case in a.cases.split(','):
                n_sites, n_samples = (int(x) for x in case.split('x'))
                d = os.path.join(root, 'species_%s' % case)
                t0 = time.perf_counter()
                synth.write_strain_species_dir(d, n_sites, n_samples, seed=4, block=max(1000, 4000000 // n_samples))
                nbytes = os.path.getsize(d + '/snps_freq.txt') + os.path.getsize(d + '/snps_depth.txt')
                say("inputs: %d sites x %d samples written in %.1f s; snps_freq.txt %.1f MB, snps_depth.txt %.1f MB"
                    % (n_sites, n_samples, time.perf_counter() - t0, os.path.getsize(d + '/snps_freq.txt') / 1e6,
                       os.path.getsize(d + '/snps_depth.txt') / 1e6))
                markers, sharing = os.path.join(root, 'markers.txt'), os.path.join(root, 'sharing.txt')
                for k in range(2):                                                   # (the first pass: warm-up)
                    t0 = time.perf_counter()
                    tables = sites.open_tables(d)
                    order = list(sites.fetch_samples(tables, zero_depth_ok=True).values())
                    cols = [s.index for s in order]
                    t1 = time.perf_counter()
                    mi, ma = strains.allele_codes(tables, 'minor_allele', n_sites), strains.allele_codes(tables, 'major_allele', n_sites)
                    res = ctx.sites_id_markers(tables.freq_text, tables.depth_text, mi, ma, cols, 0.1, 3, a.allele_prev)
                    t2 = time.perf_counter()
                    tables.write_markers(markers, res['rows'])
                    t3 = time.perf_counter()
                    listed = strains.read_markers(markers)
                    which, n_parse = strains.marker_sites(tables, listed, float('inf'))
                    t4 = time.perf_counter()
                    trk = ctx.sites_track_markers(tables.freq_text, tables.depth_text, which, cols, 0.1, 3, n_parse=n_parse)
                    t5 = time.perf_counter()
                    tables.write_pairs(sharing, cols, trk['both'])
                    t6 = time.perf_counter()
                    if k == 0:
                        continue
                    pair = sorted(ctx.sites_track_markers(tables.freq_text, tables.depth_text, which, cols, 0.1, 3, n_parse=n_parse)['ms'][5]
                                  for _ in range(a.reps))
                    say("id_markers: %d sites read, %d markers, %d group(s), cells converted by the host: %d"
                        % (res['n_sites'], len(res['rows']), res['groups'], res['side_freq'] + res['side_depth']))
                    say("  read tables  %8.3f s   device call %8.3f s   write %8.3f s (%.1f MB)" % (t1 - t0, t2 - t1, t3 - t2, os.path.getsize(markers) / 1e6))
                    say(phases(ID_PHASES, res['ms']))
                    say("  parser: %.1f MB of text in %.2f ms = %.1f GB/s" % (nbytes / 1e6, res['ms'][2], nbytes / max(res['ms'][2], 1e-9) / 1e6))
                    say("track_markers: %d sites read, %d matched, %d group(s), %d pairs of samples"
                        % (trk['n_sites'], trk['n_matched'], trk['groups'], n_samples * (n_samples - 1) // 2))
                    say("  marker list + cursor walk (host) %8.3f s   device call %8.3f s   write %8.3f s (%.1f MB)"
                        % (t4 - t3, t5 - t4, t6 - t5, os.path.getsize(sharing) / 1e6))
                    say(phases(TRACK_PHASES, trk['ms']))
                    pair_ms = pair[len(pair) // 2]
                    tiles = (n_samples + abi.SITES_PAIR_TILE - 1) // abi.SITES_PAIR_TILE
                    computed = tiles * (tiles + 1) // 2 * abi.SITES_PAIR_TILE ** 2 * ((trk['n_matched'] + 63) // 64)
                    say("  pair kernel, %d more calls: median %.3f ms (least %.3f, most %.3f); %d runs of at most %d staging steps"
                        % (a.reps, pair_ms, pair[0], pair[-1], trk['pair_runs'], trk['pair_steps']))
                    say("  pair kernel: %d word-pairs (S(S+1)/2 x words; %d and + popcount with the whole tiles) in the median = %.0f G word-pairs/s; "
                        "its input, the bit matrix, is %.2f MB" % (trk['word_pairs'], computed, trk['word_pairs'] / max(pair_ms, 1e-9) / 1e6,
                                                                  n_samples * ((trk['n_matched'] + 63) // 64) * 8 / 1e6))
                    dev = sorted(((m, p) for p, m in zip(TRACK_PHASES, trk['ms']) if p != '-' and p != 'upload+index'), reverse=True)
                    say("  largest device phases: " + ", ".join("%s %.2f ms" % (p, m) for m, p in dev[:3]))
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
