"""compare_genes.py end to end on a seeded genes directory, phase by phase.

Writes a directory in the shape of `merge_midas.py genes` output on tmpfs (midas_amd/analyze/synth.py write_genes_dir: 17-digit
reprs), then runs the command's steps as it does and prints where the time goes: mapping the matrix, the device call split
into upload + index, index, parse, bit matrix and pairs (popcount for presabs, the ordered fp64 kernel for copynum), download,
and the native writer.  Every mode is launched --reps times; each phase is the median of those launches.

The presabs pair rate is word-pairs per second -- (sample pairs with i <= j) x (64-gene words) -- the unit tools/strains_e2e.py
prints for the same kernel.  The copynum rate is (pair, gene) steps per second, printed beside the FP64 issue bound derived in
profiles/compare_genes.txt.

Two cases by default: 300 000 genes x 200 samples (the shape of tools/merge_genes_e2e.py) and 100 000 genes x 1 000 samples.

usage: python tools/compare_genes_e2e.py [--cases 300000x200,100000x1000] [--reps 9] [--dir /dev/shm] [--keep] [--out FILE]
"""
import argparse
import os
import shutil
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from midas_amd import abi  # noqa: E402
from midas_amd.analyze import synth  # noqa: E402

PHASES = ['upload+index', 'index', 'parse', 'bit matrix', 'pairs', '-', '-', 'download']
MODES = [('presabs', 'jaccard'), ('copynum', 'jaccard'), ('copynum', 'euclidean'), ('copynum', 'manhattan')]
# per (pair, gene) step and wave: jaccard 2 v_cmp_f64 + 4 v_cndmask_b32 + 2 v_add_f64; euclidean + v_add_f64 (the difference),
# v_mul_f64, v_add_f64; manhattan + v_add_f64, v_add_f64 (|x| is an input modifier).  fp64 instructions issue at half the
# fp32 rate: 4 cycles a wave on a SIMD, v_cndmask_b32 2.  1024 SIMDs at 2.4 GHz, 64 steps a wave-instruction.
ISSUE_CYCLES = {'jaccard': 2 * 4 + 4 * 2 + 2 * 4, 'euclidean': 2 * 4 + 4 * 2 + 5 * 4, 'manhattan': 2 * 4 + 4 * 2 + 4 * 4}
SIMDS, CLOCK_HZ = 1024, 2.4e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='300000x200,100000x1000')
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--dir', default='/dev/shm')
    ap.add_argument('--keep', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    root = tempfile.mkdtemp(prefix='compare_genes_e2e_', dir=a.dir)
    try:
        with abi.Context(0) as ctx:
            for case in a.cases.split(','):
                n_genes, n_samples = (int(x) for x in case.split('x'))
                d = os.path.join(root, 'species_%s' % case)
                t0 = time.perf_counter()
                synth.write_genes_dir(d, n_genes, n_samples, seed=4, block=max(1000, 4000000 // n_samples))
                path = os.path.join(d, 'genes_copynum.txt')
                say("inputs: %d genes x %d samples written in %.1f s; genes_copynum.txt %.1f MB"
                    % (n_genes, n_samples, time.perf_counter() - t0, os.path.getsize(path) / 1e6))
                t0 = time.perf_counter()
                m = abi.GenesMatrix(path)
                say("  map + header + row count (host) %.3f s" % (time.perf_counter() - t0))
                out = os.path.join(root, 'distances.txt')
                pairs_le = n_samples * (n_samples + 1) // 2
                for dtype, distance in MODES:
                    ctx.genes_compare(m.text, m.n_rows, n_samples, m.n_columns, dtype=dtype, distance=distance)      # warm-up
                    runs, wall = [], []
                    for _ in range(a.reps):
                        t0 = time.perf_counter()
                        res = ctx.genes_compare(m.text, m.n_rows, n_samples, m.n_columns, dtype=dtype, distance=distance)
                        wall.append(time.perf_counter() - t0)
                        runs.append(res['ms'])
                    med = [statistics.median(r[k] for r in runs) for k in range(8)]
                    t0 = time.perf_counter()
                    m.write_pairs(out, res)
                    t_write = time.perf_counter() - t0
                    say("%s / %s: %d rows, %d group(s) of %d rows, %d pair tile(s); median of %d launches"
                        % (dtype, distance, res['n_rows'], res['groups'], res['group_rows'], res['tiles'], a.reps))
                    say("  device call %.3f s (least %.3f, most %.3f)   write %.3f s (%.1f MB)"
                        % (statistics.median(wall), min(wall), max(wall), t_write, os.path.getsize(out) / 1e6))
                    say("  " + "  ".join("%s %.2f ms" % (p, v) for p, v in zip(PHASES, med) if p != '-' and not (p == 'bit matrix' and dtype != 'presabs')))
                    say("  parser: %.1f MB of text in %.2f ms = %.1f GB/s" % (m.text.shape[0] / 1e6, med[2], m.text.shape[0] / max(med[2], 1e-9) / 1e6))
                    pair_ms = med[4]
                    least, most = min(r[4] for r in runs), max(r[4] for r in runs)
                    if dtype == 'presabs':
                        say("  popcount pair kernel: %d word-pairs in %.3f ms (least %.3f, most %.3f) = %.0f G word-pairs/s"
                            % (res['steps'], pair_ms, least, most, res['steps'] / max(pair_ms, 1e-9) / 1e6))
                    else:
                        steps = pairs_le * res['n_rows']
                        bound = SIMDS * CLOCK_HZ * 64 / ISSUE_CYCLES[distance]
                        used = min(res['tiles'] * 4, SIMDS)
                        say("  ordered pair kernel: %d (pair, gene) steps in %.3f ms (least %.3f, most %.3f) = %.1f G steps/s; "
                            "FP64 issue bound of the whole device %.0f G steps/s, of the %d SIMDs its %d workgroups occupy %.0f G steps/s"
                            % (steps, pair_ms, least, most, steps / max(pair_ms, 1e-9) / 1e6, bound / 1e9, used, res['tiles'],
                               bound * used / SIMDS / 1e9))
                del m
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
