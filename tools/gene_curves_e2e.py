"""gene_curves.py end to end on a seeded genes directory, phase by phase.

Writes a directory in the shape of `merge_midas.py genes` output on tmpfs (midas_amd/analyze/synth.py write_pangenome_curve_dir:
genes of every sample, of all but one, of about 97, 70, 30 and 2 % of the samples, of one sample and of none), then runs the
command's steps as it does and prints where the time goes: mapping the matrix, the orders and need[] on the host, the device call
split into upload + index, index, parse, planes, the curve kernel and the download, the statistic columns and the two native
writers.  Every phase is the median of --reps launches after a warm-up launch.

The curve kernel's rate is cell steps per second -- orders x samples x genes -- for the bit-plane form (form 1) and, in one
launch, for the form that walks the parsed cells a thread an (order, gene) (form 0).  The sequential model
(tests/gene_curves_model.py) is timed on the first --model_rows rows with --model_orders orders and scaled by rows and orders;
the line says so.

usage: python tools/gene_curves_e2e.py [--cases 300000x200,100000x1000] [--orders 1000] [--reps 3] [--model_rows 1500] [--model_orders 10] [--dir /dev/shm] [--keep] [--out FILE]
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
from midas_amd.analyze import genes_curves, synth  # noqa: E402

PHASES = ['upload+index', 'index', 'parse', 'planes', 'curves', '-', '-', 'download']


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='300000x200,100000x1000')
    ap.add_argument('--orders', type=int, default=1000)
    ap.add_argument('--core_frac', type=float, default=0.95)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--model_rows', type=int, default=1500)
    ap.add_argument('--model_orders', type=int, default=10)
    ap.add_argument('--dir', default='/dev/shm')
    ap.add_argument('--keep', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    root = tempfile.mkdtemp(prefix='gene_curves_e2e_', dir=a.dir)
    try:
        with abi.Context(0) as ctx:
            for case in a.cases.split(','):
                n_genes, n_samples = (int(x) for x in case.split('x'))
                d = os.path.join(root, 'species_%s' % case)
                t0 = time.perf_counter()
                synth.write_pangenome_curve_dir(d, n_genes, n_samples, seed=4, block=max(1000, 4000000 // n_samples))
                path = os.path.join(d, 'genes_copynum.txt')
                say("inputs: %d genes x %d samples written in %.1f s; genes_copynum.txt %.1f MB"
                    % (n_genes, n_samples, time.perf_counter() - t0, os.path.getsize(path) / 1e6))
                t0 = time.perf_counter()
                m = abi.GenesMatrix(path)
                say("  map + header + row count (host) %.3f s" % (time.perf_counter() - t0))
                t0 = time.perf_counter()
                orders = genes_curves.orders_table(range(n_samples), a.orders, 0)
                need = genes_curves.need_table(n_samples, a.core_frac)
                say("  %d orders and need[] (host) %.4f s" % (a.orders, time.perf_counter() - t0))
                call = lambda form: abi.genes_curves(ctx, m.text, m.n_rows, n_samples, m.n_columns, orders, need, form=form)
                steps = (1 + a.orders) * n_samples * m.n_rows
                first = None
                for form in (1, 0):
                    if form == 1:
                        call(form)                                                                            # warm-up
                    runs, wall = [], []
                    for _ in range(a.reps if form == 1 else 1):
                        t0 = time.perf_counter()
                        res = call(form)
                        wall.append(time.perf_counter() - t0)
                        runs.append(res['ms'])
                    med = [statistics.median(r[k] for r in runs) for k in range(8)]
                    if form == 0:
                        same = all((res[k] == first[k]).all() for k in ('pan', 'core', 'single'))
                        say("  form 0 (a thread an (order, gene), plain counts over the cells), one launch: curves %.2f ms = %.1f G cell steps/s; "
                            "arrays equal to form 1's: %s" % (med[4], steps / max(med[4], 1e-9) / 1e6, same))
                        continue
                    first = res
                    say("core_frac %s: %d rows, %d group(s) of %d rows, %d samples in use, %d orders, %d counter planes, %d words in the last group; "
                        "median of %d launches"
                        % (repr(a.core_frac), res['n_rows'], res['groups'], res['group_rows'], res['n_used'], res['n_orders'], res['planes'],
                           res['words'], a.reps))
                    say("  device call %.3f s (least %.3f, most %.3f)" % (statistics.median(wall), min(wall), max(wall)))
                    say("  " + "  ".join("%s %.2f ms" % (p, v) for p, v in zip(PHASES, med) if p != '-'))
                    say("  parser: %.1f MB of text in %.2f ms = %.1f GB/s" % (m.text.shape[0] / 1e6, med[2], m.text.shape[0] / max(med[2], 1e-9) / 1e6))
                    say("  curve kernel: %d cell steps in %.3f ms (least %.3f, most %.3f) = %.1f G cell steps/s"
                        % (steps, med[4], min(r[4] for r in runs), max(r[4] for r in runs), steps / max(med[4], 1e-9) / 1e6))
                    t0 = time.perf_counter()
                    table = genes_curves.table_columns(res)
                    t_table = time.perf_counter() - t0
                    out, per_order = os.path.join(root, 'curves.txt'), os.path.join(root, 'orders.txt')
                    t0 = time.perf_counter()
                    m.write_curves(out, res, table)
                    t_out = time.perf_counter() - t0
                    t0 = time.perf_counter()
                    m.write_curve_orders(per_order, res, orders)
                    say("  statistic columns (host) %.3f s   write curves %.3f s (%.2f MB)   write orders %.3f s (%.1f MB)"
                        % (t_table, t_out, os.path.getsize(out) / 1e6, time.perf_counter() - t0, os.path.getsize(per_order) / 1e6))
                    say("  " + genes_curves.heaps_line(table['new_mean'].tolist() if a.orders else []))
                if a.model_rows > 0:
                    from tests import compare_genes_model as CG
                    from tests import gene_curves_model as M
                    rows, few = min(a.model_rows, m.n_rows), min(a.model_orders, 1 + a.orders)
                    t0 = time.perf_counter()
                    cells, _ = CG.read_cells(m.text, rows, n_samples, m.n_columns)
                    t_read = time.perf_counter() - t0
                    t0 = time.perf_counter()
                    M.curves(cells, 0.35, orders[:few], need.tolist())
                    t_model = time.perf_counter() - t0
                    scale = (m.n_rows / rows) * ((1 + a.orders) / few)
                    say("  sequential model (numpy cumsum) on the first %d rows and %d orders: cells %.2f s, curves %.3f s; SCALED by rows and "
                        "orders to the whole call (x %.0f), not run: %.0f s" % (rows, few, t_read, t_model, scale, t_model * scale))
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
