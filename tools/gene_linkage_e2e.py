"""gene_linkage.py end to end on a seeded genes directory, phase by phase.

Writes a directory in the shape of `merge_midas.py genes` output on tmpfs (midas_amd/analyze/synth.py write_linked_genes_dir:
independent genes at mixed prevalence and planted groups of 5 to 50 genes), then runs the command's steps as it does and prints
where the time goes: mapping the matrix, the device call split into upload + index, index, parse, planes, the pair kernel's count
pass and write pass, the labels, download, and the two native writers.  Every phase is the median of --reps launches after a
warm-up launch.

The pair kernel's rate is word-pairs per second -- (pairs of kept genes) x (64-sample words) a pass -- the unit
tools/compare_genes_e2e.py prints for ss_pairs_kernel (profiles/compare_genes.txt); the shapes differ, so that is context.  The
form that reads both sides word by word (pair_form 1) is timed beside the register form, in one launch.  The sequential model
(tests/gene_linkage_model.py) is timed on the first --model_rows rows and scaled by the number of pairs; the line says so.

usage: python tools/gene_linkage_e2e.py [--cases 100000x1000,300000x200] [--reps 3] [--model_rows 1500] [--dir /dev/shm] [--keep] [--out FILE]
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
from midas_amd.analyze import genes_linkage, synth  # noqa: E402

PHASES = ['upload+index', 'index', 'parse', 'planes', 'count pass', 'write pass', 'labels', 'download']


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='100000x1000,300000x200')
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--min_jaccard', type=float, default=0.9)
    ap.add_argument('--model_rows', type=int, default=1500)
    ap.add_argument('--dir', default='/dev/shm')
    ap.add_argument('--keep', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    root = tempfile.mkdtemp(prefix='gene_linkage_e2e_', dir=a.dir)
    try:
        with abi.Context(0) as ctx:
            for case in a.cases.split(','):
                n_genes, n_samples = (int(x) for x in case.split('x'))
                d = os.path.join(root, 'species_%s' % case)
                t0 = time.perf_counter()
                synth.write_linked_genes_dir(d, n_genes, n_samples, seed=4, block=max(1000, 4000000 // n_samples))
                path = os.path.join(d, 'genes_copynum.txt')
                say("inputs: %d genes x %d samples written in %.1f s; genes_copynum.txt %.1f MB"
                    % (n_genes, n_samples, time.perf_counter() - t0, os.path.getsize(path) / 1e6))
                t0 = time.perf_counter()
                m = abi.GenesMatrix(path)
                say("  map + header + row count (host) %.3f s" % (time.perf_counter() - t0))
                t0 = time.perf_counter()
                need = genes_linkage.need_table(n_samples, a.min_jaccard)
                say("  need[] by bisection (host) %.4f s" % (time.perf_counter() - t0))
                words = (n_samples + 63) // 64
                for form in (0, 1):
                    if form == 0:
                        ctx.genes_linkage(m.text, m.n_rows, n_samples, m.n_columns, need, pair_form=form)      # warm-up
                    runs, wall = [], []
                    for _ in range(a.reps if form == 0 else 1):
                        t0 = time.perf_counter()
                        res = ctx.genes_linkage(m.text, m.n_rows, n_samples, m.n_columns, need, pair_form=form)
                        wall.append(time.perf_counter() - t0)
                        runs.append(res['ms'])
                    med = [statistics.median(r[k] for r in runs) for k in range(8)]
                    word_pairs = res['visited'] * words
                    if form == 1:
                        say("  the form for any width (both sides word by word from memory), one launch: count pass %.2f ms, write pass %.2f ms = %.0f G word-pairs/s"
                            % (med[4], med[5], word_pairs / max(med[4], 1e-9) / 1e6))
                        continue
                    say("min_jaccard %s: %d rows, %d group(s) of %d rows, %d kept genes, %d pairs visited, %d linked, %d strips, %d words in registers, "
                        "%d label rounds; median of %d launches"
                        % (repr(a.min_jaccard), res['n_rows'], res['groups'], res['group_rows'], res['n_kept'], res['visited'], res['linked'],
                           res['strips'], res['form'], res['label_rounds'], a.reps))
                    say("  device call %.3f s (least %.3f, most %.3f)" % (statistics.median(wall), min(wall), max(wall)))
                    say("  " + "  ".join("%s %.2f ms" % (p, v) for p, v in zip(PHASES, med)))
                    say("  parser: %.1f MB of text in %.2f ms = %.1f GB/s" % (m.text.shape[0] / 1e6, med[2], m.text.shape[0] / max(med[2], 1e-9) / 1e6))
                    say("  pair kernel, count pass: %d word-pairs in %.3f ms (least %.3f, most %.3f) = %.0f G word-pairs/s; write pass %.3f ms: "
                        "the two passes cost %.2f x the count pass"
                        % (word_pairs, med[4], min(r[4] for r in runs), max(r[4] for r in runs), word_pairs / max(med[4], 1e-9) / 1e6, med[5],
                           (med[4] + med[5]) / max(med[4], 1e-9)))
                    out, grp = os.path.join(root, 'pairs.txt'), os.path.join(root, 'groups.txt')
                    t0 = time.perf_counter()
                    m.write_linkage(out, res)
                    t_pairs = time.perf_counter() - t0
                    t0 = time.perf_counter()
                    n_groups = m.write_groups(grp, res, 2)
                    say("  write pairs %.3f s (%.1f MB)   write groups %.3f s (%d groups, %.1f MB)"
                        % (t_pairs, os.path.getsize(out) / 1e6, time.perf_counter() - t0, n_groups, os.path.getsize(grp) / 1e6))
                    visited = res['visited']
                if a.model_rows > 0:
                    from tests import compare_genes_model as CG
                    from tests import gene_linkage_model as M
                    rows = min(a.model_rows, m.n_rows)
                    t0 = time.perf_counter()
                    cells, _ = CG.read_cells(m.text, rows, n_samples, m.n_columns)
                    t_read = time.perf_counter() - t0
                    t0 = time.perf_counter()
                    mod = M.link(cells, 0.35, 2, 2, need.tolist())
                    t_link = time.perf_counter() - t0
                    say("  sequential model on the first %d rows: cells %.2f s, %d pairs in %.2f s; SCALED by pairs to the whole matrix (x %.0f): %.0f s"
                        % (rows, t_read, mod['visited'], t_link, visited / max(mod['visited'], 1), t_link * visited / max(mod['visited'], 1)))
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
