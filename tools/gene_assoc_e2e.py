"""gene_assoc.py end to end on a seeded genes directory, phase by phase.

Writes a directory in the shape of `merge_midas.py genes` output on tmpfs (midas_amd/analyze/synth.py write_assoc_genes_dir:
genes independent of the label at mixed prevalence, one in a hundred planted) with its groups file, then runs the command's
steps as it does and prints where the time goes: the relabellings on the host, the device call split into upload + index,
parse, keep + ranks, the product (form 1, the i8 MFMA kernel; form 0, one thread a (gene, relabelling) with plain adds, timed by
itself), download, then the p-values on the host and the native writer.  Every phase is the median of --reps launches after a
warm-up launch; form 0 is launched once, and not at all where its time at a tenth of the relabellings says that one launch
would take more than --form0_limit seconds (the line says so).  Both forms must leave the same exceed counts.

The product's rate is multiply-adds per second: kept genes x used samples x relabellings (the padding to the tiles not
counted).  The sequential model (tests/gene_assoc_model.py) is timed on the first --model_rows rows with --model_perms
relabellings and scaled by rows and relabellings; the line says "scaled, not run".

usage: python tools/gene_assoc_e2e.py [--cases 300000x200,100000x1000] [--perms 1000,10000] [--reps 3] [--model_rows 1500] [--dir /dev/shm] [--out FILE]
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
from midas_amd.analyze import genes_assoc, synth  # noqa: E402

PHASES = ['upload+index', 'index', 'parse', 'keep+ranks', 'product', 'expand', '-', 'download']


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='300000x200,100000x1000')
    ap.add_argument('--perms', default='1000,10000')
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--form0_limit', type=float, default=60.0)
    ap.add_argument('--model_rows', type=int, default=1500)
    ap.add_argument('--model_perms', type=int, default=100)
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

    root = tempfile.mkdtemp(prefix='gene_assoc_e2e_', dir=a.dir)
    perms = [int(x) for x in a.perms.split(',')]
    try:
        with abi.Context(0) as ctx:
            for case in a.cases.split(','):
                n_genes, n_samples = (int(x) for x in case.split('x'))
                d = os.path.join(root, 'species_%s' % case)
                t0 = time.perf_counter()
                info = synth.write_assoc_genes_dir(d, n_genes, n_samples, seed=4, block=max(1000, 4000000 // n_samples))
                path = os.path.join(d, 'genes_copynum.txt')
                say("inputs: %d genes x %d samples written in %.1f s; genes_copynum.txt %.1f MB"
                    % (n_genes, n_samples, time.perf_counter() - t0, os.path.getsize(path) / 1e6))
                t0 = time.perf_counter()
                m = abi.GenesMatrix(path)
                used, cases, controls, _, _ = genes_assoc.read_groups(info['groups_path'], m.sample_ids)
                say("  map + header + row count + groups file (host) %.3f s: %d used samples, %d cases" % (time.perf_counter() - t0, len(used), len(cases)))
                use, cs = genes_assoc.words_of(used, n_samples), genes_assoc.words_of(cases, n_samples)
                for dtype in ('presabs', 'copynum'):
                    walk_ms = {}
                    for P in perms:
                        t0 = time.perf_counter()
                        planes = genes_assoc.permutation_planes(used, len(cases), P, 0, n_samples)
                        t_planes = time.perf_counter() - t0
                        call = lambda form: ctx.genes_assoc(m.text, m.n_rows, n_samples, m.n_columns, use, cs, planes, dtype=dtype, form=form)
                        call(1)                                        # warm-up
                        runs, wall = [], []
                        for _ in range(a.reps):
                            t0 = time.perf_counter()
                            res = call(1)
                            wall.append(time.perf_counter() - t0)
                            runs.append(res['ms'])
                        med = [statistics.median(r[k] for r in runs) for k in range(8)]
                        macs = res['n_kept'] * res['n_used'] * P
                        say("%s, %d relabellings: %d rows, %d group(s) of %d rows, %d kept genes, digits %s; median of %d launches"
                            % (dtype, P, res['n_rows'], res['groups'], res['group_rows'], res['n_kept'], 'in LDS' if res['in_lds'] else 'from memory', a.reps))
                        say("  relabellings on the host %.3f s   device call %.3f s (least %.3f, most %.3f): " % (t_planes, statistics.median(wall), min(wall), max(wall))
                            + "  ".join("%s %.2f ms" % (p, v) for p, v in zip(PHASES, med) if p != '-'))
                        say("  product, form 1 (i8 MFMA): %.3g multiply-adds in %.3f ms (least %.3f, most %.3f) = %.2f T multiply-adds/s"
                            % (macs, med[4], min(r[4] for r in runs), max(r[4] for r in runs), macs / max(med[4], 1e-9) / 1e9))
                        guess = walk_ms.get(P // 10, 0.0) * 10 / 1e3
                        if guess > a.form0_limit:
                            say("  product, form 0 (plain adds): SKIPPED, not run: %.1f s at %d relabellings says about %.0f s here, more than %.0f s"
                                % (walk_ms[P // 10] / 1e3, P // 10, guess, a.form0_limit))
                        else:
                            r0 = call(0)
                            walk_ms[P] = r0['ms'][4]
                            assert np.array_equal(r0['exceed'], res['exceed']) and np.array_equal(r0['w'], res['w'])
                            say("  product, form 0 (plain adds), one launch: %.1f ms = %.3f T multiply-adds/s: form 1 is %.0f x faster; the same exceed counts"
                                % (r0['ms'][4], macs / max(r0['ms'][4], 1e-9) / 1e9, r0['ms'][4] / max(med[4], 1e-9)))
                        tp, tw = [], []
                        out = os.path.join(root, 'assoc.txt')
                        for _ in range(a.reps):
                            t0 = time.perf_counter()
                            table = genes_assoc.table_columns(res)
                            tp.append(time.perf_counter() - t0)
                            t0 = time.perf_counter()
                            m.write_assoc(out, res, table)
                            tw.append(time.perf_counter() - t0)
                        planted = info['planted'][res['row_of_slot']]
                        say("  p-values + q-values (host) %.3f s   write %.3f s (%.1f MB)   q_value < 0.05: %d of %d planted, %d of %d others; q_perm < 0.05: %d and %d"
                            % (statistics.median(tp), statistics.median(tw), os.path.getsize(out) / 1e6, int((table['q_value'][planted] < 0.05).sum()),
                               int(planted.sum()), int((table['q_value'][~planted] < 0.05).sum()), int((~planted).sum()),
                               int((table['q_perm'][planted] < 0.05).sum()), int((table['q_perm'][~planted] < 0.05).sum())))
                    if a.model_rows > 0:
                        from tests import compare_genes_model as CG
                        from tests import gene_assoc_model as M
                        rows = min(a.model_rows, m.n_rows)
                        t0 = time.perf_counter()
                        cells, _ = CG.read_cells(m.text, rows, n_samples, m.n_columns)
                        t_read = time.perf_counter() - t0
                        small = genes_assoc.permutation_planes(used, len(cases), a.model_perms, 0, n_samples)
                        t0 = time.perf_counter()
                        M.stats(cells, used, cases, small, dtype=dtype)
                        t_model = time.perf_counter() - t0
                        scale = m.n_rows / rows * perms[-1] / a.model_perms
                        say("  sequential model (%s) on the first %d rows with %d relabellings: cells %.2f s, statistics %.2f s; scaled, not run, to %d rows "
                            "and %d relabellings (x %.0f): %.0f s" % (dtype, rows, a.model_perms, t_read, t_model, m.n_rows, perms[-1], scale, t_model * scale))
                del m
                if not a.keep:
                    shutil.rmtree(d, ignore_errors=True)
    finally:
        if not a.keep:
            shutil.rmtree(root, ignore_errors=True)


if __name__ == '__main__':
    main()
