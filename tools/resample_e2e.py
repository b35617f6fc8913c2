"""snp_diversity.py --rand_reads N --replace_reads end to end on a seeded species directory (default 2 000 000 sites x 50 samples,
analyze/synth.write_species_dir on tmpfs): medians of --reps runs with their spread (min .. max) of
  * the whole command, as a process: with --rand_reads N --replace_reads --seed 1, without --rand_reads, and -- given --parent,
    the scripts/snp_diversity.py of another checkout -- that checkout's command without --rand_reads, run alternately with ours;
  * the phases of the device call with --rand_reads: site, eligibility, generate, compact, resample, re-pool, sums;
  * the one-workgroup generator's raw words per second, and the cells that drew;
  * what the comparison is against: this box's HOST producing as many raw words (RandomState.randint(0, 2**32, n, dtype=uint32),
    measured on a piece of 2^26 words and scaled) plus their upload to the device (torch, when it is there).

usage: python tools/resample_e2e.py [--sites 2000000] [--samples 50] [--reads 20] [--reps 5] [--parent PATH] [--dir /dev/shm] [--out FILE]
"""
import argparse
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from midas_amd import abi  # noqa: E402
from midas_amd.analyze import cli, diversity, sites, synth  # noqa: E402

DRAW_PHASES = ['eligibility', 'generate', 'compact', 'resample', 're-pool']


class Shared:
    def __init__(self, ctx):
        self._ctx = ctx

    def sites_scan(self, *a, **kw):
        return self._ctx.sites_scan(*a, **kw)

    def close(self):
        pass


def med(v):
    return "%.3f (%.3f .. %.3f)" % (statistics.median(v), min(v), max(v))


def command_seconds(script, argv):
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, script] + argv, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        raise SystemExit("%s failed:\n%s" % (script, r.stderr))
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sites', type=int, default=2000000)
    ap.add_argument('--samples', type=int, default=50)
    ap.add_argument('--reads', type=int, default=20)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--parent', default=None)
    ap.add_argument('--dir', default='/dev/shm')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    root = tempfile.mkdtemp(prefix='resample_e2e_', dir=a.dir)
    try:
        d = os.path.join(root, 'species_1')
        synth.write_species_dir(d, a.sites, a.samples, seed=4)
        out = os.path.join(root, 'out.txt')
        ours = os.path.join(ROOT, 'scripts', 'snp_diversity.py')
        rr = ['--rand_reads', str(a.reads), '--replace_reads', '--seed', '1']
        say("inputs: %d sites x %d samples; medians of %d with (min .. max)" % (a.sites, a.samples, a.reps))
        # ---- the whole command ------------------------------------------------------------------------------------------------
        command_seconds(ours, [d, '--out', out])                                         # (warm-up: page cache, code objects)
        with_rr, plain, parent = [], [], []
        for _ in range(a.reps):
            plain.append(command_seconds(ours, [d, '--out', out]))
            if a.parent:
                parent.append(command_seconds(a.parent, [d, '--out', out]))
            with_rr.append(command_seconds(ours, [d, '--out', out] + rr))
        say("whole command, --rand_reads %d --replace_reads: %s s" % (a.reads, med(with_rr)))
        say("whole command, no --rand_reads:                %s s" % med(plain))
        if a.parent:
            say("whole command, no --rand_reads, parent commit: %s s" % med(parent))
        # ---- the phases -------------------------------------------------------------------------------------------------------
        args = cli.diversity_arguments([d, '--out', out] + rr)
        tables = sites.open_tables(d)
        samples = sites.fetch_samples(tables)
        ms, draw, res = [], [], None
        with abi.Context(0) as ctx:
            for k in range(a.reps + 1):
                np.random.seed(1)
                res = diversity.compute(args, tables, samples, Shared(ctx))
                if k:
                    ms.append(res['ms'])
                    draw.append(res['draw_ms'])
        say("device call with --rand_reads %d: %d sites kept, %d resampled, %d cells drew, %d group(s); raw words generated %d, consumed %d, accepted used %d"
            % (a.reads, res['n_kept'], res['n_resampled'], res['n_drew'], res['groups'], res['raw_made'], res['raw_consumed'], res['accepted_used']))
        say("  site        %s ms" % med([m[3] for m in ms]))
        for j, name in enumerate(DRAW_PHASES):
            say("  %-11s %s ms" % (name, med([x[j] for x in draw])))
        say("  sums        %s ms" % med([m[5] for m in ms]))
        gen = [res['raw_made'] / (x[1] * 1e-3) / 1e6 for x in draw if x[1] > 0]
        if gen:
            say("generator (one workgroup): %s M raw words / s" % med(gen))
        # ---- the host, for as many raw words ----------------------------------------------------------------------------------
        piece = 1 << 26
        try:
            import torch
            up = torch.cuda.is_available()
        except ImportError:
            up = False
        host, upload = [], []
        rs = np.random.RandomState(1)
        for _ in range(a.reps):
            t0 = time.perf_counter()
            w = rs.randint(0, 2 ** 32, piece, dtype=np.uint32)
            t1 = time.perf_counter()
            if up:
                g = torch.from_numpy(w.view(np.int32)).cuda()
                torch.cuda.synchronize()
                del g
            host.append(t1 - t0)
            upload.append(time.perf_counter() - t1)
        scale = res['raw_made'] / piece
        say("host, RandomState.randint(0, 2**32, 2^26, dtype=uint32): %s s a piece = %s M words / s" % (med(host), med([piece / x / 1e6 for x in host])))
        say("host, upload of a piece%s: %s s" % ('' if up else ' (no torch device: not measured)', med(upload)))
        say("host, scaled to the %d raw words of this run: %.3f s generate + %.3f s upload; device generate %.3f s"
            % (res['raw_made'], statistics.median(host) * scale, statistics.median(upload) * scale, statistics.median([x[1] for x in draw]) * 1e-3))
    finally:
        shutil.rmtree(root, ignore_errors=True)
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
