"""`run_midas.py genes` from the aligner's SAM (read_sam(order='file') + midas_genes_count_device) beside the BAM route (host
decode + pack_records + the device call of midas_genes_count), phase by phase, on the README's genes shape: about 3.4 M reads
of 150 bases over 40 000 genes.

The reads are a seeded pangenome dataset tiled up to the wanted count (the per-gene answer of both routes is compared, so the
tiling cannot hide a difference), written once as SAM text and once as a BAM, in the same order.  Printed per route, best of
--reps: the decode (the SAM decode's own phases from midas_sam_decode_timing), the device call split into the facts kernel
and filter + sort + sums (midas_genes_count_timing), and for the BAM route the host's pass (whole call minus its device time).
Times are host clocks around calls that end in a stream synchronise, or device events where the library hands them out.

usage: python tools/genes_sam_e2e.py [--reads 3400000] [--genes 40000] [--reps 3] [--dir /dev/shm] [--out FILE]
"""
import argparse
import os
import shutil
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from midas_amd import abi, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reads', type=int, default=3400000)
    ap.add_argument('--genes', type=int, default=40000)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--dir', default='/dev/shm')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    n_species = 10
    t0 = time.perf_counter()
    seed_reads = max(1000, min(a.reads, 200000))
    ds = synth.make_pangenome_dataset(n_species=n_species, genes_per_species=max(4, a.genes // n_species), n_reads=seed_reads, seed=31,
                                      silent_fraction=0.0)
    base_n = int(ds['reads'].n_reads)
    times = max(1, -(-a.reads // base_n))
    pick = np.tile(np.arange(base_n), times)[:max(a.reads, base_n)]
    pick = pick[np.random.default_rng(2).permutation(pick.size)]
    reads, refid = synth.take_reads(ds['reads'], pick), np.ascontiguousarray(ds['refid'][pick])
    names, lengths = ds['gene_ids'], [len(s) for s in ds['gene_seq']]
    thr = abi.Thresholds.from_args(dict(abi.DEFAULT_ARGS, mapid=94.0, readq=20, mapq=0, aln_cov=0.75))
    root = tempfile.mkdtemp(prefix='genes_sam_e2e_', dir=a.dir)
    try:
        sam, bam = os.path.join(root, 'pangenomes.sam'), os.path.join(root, 'pangenomes.bam')
        synth.write_sam(sam, names, lengths, reads, refid)
        abi.write_bam(bam, names, lengths, refid, reads)
        say("%d reads over %d genes; pangenomes.sam %.1f MB, pangenomes.bam %.1f MB; made and written in %.1f s"
            % (reads.n_reads, len(names), os.path.getsize(sam) / 1e6, os.path.getsize(bam) / 1e6, time.perf_counter() - t0))
        del reads
        with abi.Context(0) as ctx:
            say("device: %s" % ctx.device_info().get('name', '?'))
            best = {}
            answers = {}
            for rep in range(a.reps):
                # ---- SAM: text -> device columns in file order -> facts, filter, sort, sums on the device
                t0 = time.perf_counter()
                _, _, rid, dreads = abi.read_sam(sam, ctx, order='file')
                t1 = time.perf_counter()
                out = ctx.genes_count_device(thr, dreads, rid, lengths)
                t2 = time.perf_counter()
                row = dict(decode=(t1 - t0) * 1e3, call=(t2 - t1) * 1e3, phases=abi.sam_decode_timing(ctx), device=ctx.genes_count_timing())
                if 'sam' not in best or row['decode'] + row['call'] < best['sam']['decode'] + best['sam']['call']:
                    best['sam'] = row
                answers['sam'] = out[:3]
                del dreads, rid
                # ---- BAM: host decode -> pack_records on the host's cores -> filter, sort, sums on the device
                t0 = time.perf_counter()
                _, _, rid, hreads = abi.read_bam(bam)
                t1 = time.perf_counter()
                out = ctx.genes_count(thr, hreads, rid, lengths)
                t2 = time.perf_counter()
                row = dict(decode=(t1 - t0) * 1e3, call=(t2 - t1) * 1e3, device_ms=out[3])
                if 'bam' not in best or row['decode'] + row['call'] < best['bam']['decode'] + best['bam']['call']:
                    best['bam'] = row
                answers['bam'] = out[:3]
                del hreads, rid
            same = all(np.array_equal(x, y) for x, y in zip(answers['sam'][:2], answers['bam'][:2])) and \
                answers['sam'][2].tobytes() == answers['bam'][2].tobytes()
            say("per-gene aligned / mapped / depth of the two routes identical: %s" % same)
            s, b = best['sam'], best['bam']
            say("\nSAM route (read_sam(order='file') + genes_count_device), best of %d: %.1f ms" % (a.reps, s['decode'] + s['call']))
            say("  decode                         %9.2f ms" % s['decode'])
            for k in abi.SAM_PHASES:
                say("    %-28s %9.2f ms" % (k, s['phases'][k]))
            say("  device call, whole             %9.2f ms   (small columns up: 29 B a read; results down)" % s['call'])
            say("    facts kernel                 %9.3f ms   (device events)" % s['device']['facts kernel'])
            say("    filter + sort + sums         %9.3f ms   (device events)" % s['device']['filter + sort + sums'])
            say("\nBAM route (read_bam on the host + genes_count), best of %d: %.1f ms" % (a.reps, b['decode'] + b['call']))
            say("  host BGZF decode               %9.2f ms" % b['decode'])
            say("  genes_count, whole             %9.2f ms" % b['call'])
            say("    filter + sort + sums         %9.3f ms   (device events)" % b['device_ms'])
            say("    pack_records + copies        %9.2f ms   (whole call minus the device events)" % (b['call'] - b['device_ms']))
    finally:
        shutil.rmtree(root, ignore_errors=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write("\n".join(lines) + "\n")


if __name__ == '__main__':
    main()
