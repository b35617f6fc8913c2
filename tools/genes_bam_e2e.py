"""`run_midas.py genes --call_genes` over pangenomes.bam by its two routes, whole count_mapped_bp each: the host route (read_bam on
the host's threads + midas_genes_count: --device_inflate off) beside the one-pass device route (midas_genes_count_bam:
--device_inflate on), on seeded pangenome BAMs of the README's genes shape -- 3.4 M reads of 150 bases over 40 000 genes -- and
of one tenth and ten times that (reads and genes alike).

The reads are a seeded pangenome dataset tiled up to the wanted count and shuffled (aligner order).  At every size the two routes
take turns in one process: one warm-up each, then --reps runs each; printed is median [min .. max] of the whole count_mapped_bp
(host clock: file to folded per-gene numbers) and the medians of the device route's laps (midas_genes_count_bam's out_ms8).  The
three per-gene arrays of the two routes must be equal to the byte at every size, or the tool fails.  It needs a GPU: without
one abi.Context raises and the tool ends there.

The last line per size applies the rule of `--device_inflate auto` (midas_amd/run/genes.py AUTO_DEVICE_BAM_BYTES): the device
route wins a size when its median lies below the host route's by more than the spread (max - min) of either route's runs.

usage: python tools/genes_bam_e2e.py [--scales 0.1,1,10] [--reads 3400000] [--genes 40000] [--reps 7] [--dir /dev/shm] [--out FILE]
"""
import argparse
import contextlib
import io
import os
import shutil
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from midas_amd import abi, synth  # noqa: E402
from midas_amd.run import genes as run_genes  # noqa: E402


def _sample(root, n_reads, n_genes):
    """pangenomes.bam under root/genes/temp -> (gene ids, their species, lengths, records, bytes of the file)."""
    n_species = 10
    seed_reads = max(1000, min(n_reads, 200000))
    ds = synth.make_pangenome_dataset(n_species=n_species, genes_per_species=max(4, n_genes // n_species), n_reads=seed_reads, seed=31,
                                      silent_fraction=0.0)
    base_n = int(ds['reads'].n_reads)
    pick = np.tile(np.arange(base_n), max(1, -(-n_reads // base_n)))[:max(n_reads, base_n)]
    pick = pick[np.random.default_rng(2).permutation(pick.size)]
    reads, refid = synth.take_reads(ds['reads'], pick), np.ascontiguousarray(ds['refid'][pick])
    lengths = [len(s) for s in ds['gene_seq']]
    os.makedirs(os.path.join(root, 'genes', 'temp'))
    path = os.path.join(root, 'genes', 'temp', 'pangenomes.bam')
    abi.write_bam(path, ds['gene_ids'], lengths, refid, reads)
    return list(ds['gene_ids']), list(ds['gene_species']), lengths, int(reads.n_reads), os.path.getsize(path)


def _fresh(gene_ids, gene_species, lengths):
    species, genes = {}, {}
    for gid, sp, ln in zip(gene_ids, gene_species, lengths):
        if sp not in species:
            species[sp] = run_genes.Species(sp)
        species[sp].pangenome_size += 1
        genes[gid] = run_genes.Gene(gid, sp, ln)
    return species, genes


def _run(ctx, root, mode, gene_ids, gene_species, lengths):
    """One count_mapped_bp by `mode` (--device_inflate) -> (milliseconds, the three per-gene arrays, the route's log line)."""
    species, genes = _fresh(gene_ids, gene_species, lengths)
    log = io.StringIO()
    args = dict(outdir=root, mapid=94.0, readq=20, mapq=0, aln_cov=0.75, device_inflate=mode, log=log)
    with contextlib.redirect_stdout(io.StringIO()):
        t0 = time.perf_counter()
        run_genes.count_mapped_bp(args, species, genes, ctx)
        ms = (time.perf_counter() - t0) * 1e3
    arrays = (np.array([genes[g].aligned_reads for g in gene_ids], np.int64), np.array([genes[g].mapped_reads for g in gene_ids], np.int64),
              np.array([genes[g].depth for g in gene_ids], np.float64))
    return ms, arrays, log.getvalue().strip()


def _spread(v):
    return "%9.1f [%9.1f .. %9.1f]" % (float(np.median(v)), min(v), max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--scales', default='0.1,1,10')
    ap.add_argument('--reads', type=int, default=3400000)
    ap.add_argument('--genes', type=int, default=40000)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--dir', default='/dev/shm')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    out = None
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        out = open(a.out, 'w')

    def say(s):
        print(s, flush=True)
        if out:             # (line by line: a size that does not finish leaves the ones before it)
            out.write(s + "\n")
            out.flush()

    with abi.Context(0) as ctx:         # (no GPU: this raises, and nothing below runs)
        say("device: %s; the host route's threads: a CPU budget of %d (the process may run on %d)"
            % (ctx.device_info().get('name', '?'), abi.load_library().midas_snps_cpu_budget(), len(os.sched_getaffinity(0))))
        for scale in (float(x) for x in a.scales.split(',')):
            root = tempfile.mkdtemp(prefix='genes_bam_e2e_', dir=a.dir)
            try:
                t0 = time.perf_counter()
                gene_ids, gene_species, lengths, n, size = _sample(root, int(a.reads * scale), int(a.genes * scale))
                say("\n== %d reads over %d genes; pangenomes.bam %.1f MB (%d bytes); made and written in %.1f s"
                    % (n, len(gene_ids), size / 1e6, size, time.perf_counter() - t0))
                ms = {'off': [], 'on': []}
                laps = []
                first = {}
                for rep in range(a.reps + 1):           # (rep 0: the warm-up of both)
                    for mode in ('off', 'on'):
                        t, arrays, line = _run(ctx, root, mode, gene_ids, gene_species, lengths)
                        if rep == 0:
                            first[mode] = arrays
                            say("  %-3s: %s" % (mode, line))
                            continue
                        ms[mode].append(t)
                        if mode == 'on':
                            laps.append(ctx.genes_count_bam_timing())
                        if not all(x.tobytes() == y.tobytes() for x, y in zip(arrays, first['off'])):
                            sys.exit("the %s route's per-gene arrays differ from the host route's at %d reads" % (mode, n))
                if not all(x.tobytes() == y.tobytes() for x, y in zip(first['on'], first['off'])):
                    sys.exit("the device route's per-gene arrays differ from the host route's at %d reads" % n)
                say("  per-gene aligned / mapped / depth of the two routes equal to the byte: True (%d runs each)" % (a.reps + 1))
                say("  whole count_mapped_bp, ms, median [min .. max] of %d:" % a.reps)
                say("    host route   (--device_inflate off)  %s" % _spread(ms['off']))
                say("    device route (--device_inflate on)   %s" % _spread(ms['on']))
                say("  device route's laps, ms, median of %d:" % a.reps)
                for k in abi.GENES_BAM_PHASES:
                    say("    %-28s %9.3f" % (k, float(np.median([l[0][k] for l in laps]))))
                say("    %s" % ', '.join("%s %d" % (k, laps[-1][1][k]) for k in abi.GENES_BAM_STATS))
                spread = max(max(ms['off']) - min(ms['off']), max(ms['on']) - min(ms['on']))
                gain = float(np.median(ms['off']) - np.median(ms['on']))
                say("  auto's rule: host median - device median = %.1f ms, the larger spread (max - min) of the two = %.1f ms: the %s route takes this size"
                    % (gain, spread, 'device' if gain > spread else 'host'))
            finally:
                shutil.rmtree(root, ignore_errors=True)
    if out:
        out.close()


if __name__ == '__main__':
    main()
