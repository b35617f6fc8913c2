"""The SAM decode (run_midas.py snps --sam; midas_sam_load_device, midas_sam_load_resident) end to end on bench.py's workloads, phase
by phase, in both forms over the same file in one run: columns (read_sam -> batch create -> first run; the baseline) and resident
(read_sam(resident=True) -> batch over the handle's records -> first run).  Per form: every rep's times, the decode's phases, the
medians with min and max, and the free device memory when the decode and the batch are resident together; then whether the
resident form's median from file to batch ready is ahead of the column form's by more than that form's own min-max spread.

For configs[1] and configs[2] of bench.py's generator (synth.CONFIGS c2, c3) the reads are written as SAM text in a random order
-- as the aligner leaves them -- and as the coordinate-sorted BAM the reference's pipeline would have made of them.  Printed:
the phases of the decode (map + header, upload, line index, pass 1, scans, pass 2, sort + gather, columns down; host clock
around stream synchronisations), the whole against read_bam(resident=True) of the same reads, GB/s of text, and the one
expectation held against the numbers: upload + pass 2 beside the time the same bytes take over the link from page-locked
memory (the HIP runtime through ctypes, same process).

usage: python tools/sam_e2e.py [--configs c2,c3] [--reps 7] [--dir /dev/shm] [--out FILE]
"""
import argparse
import os
import shutil
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from midas_amd import abi, synth, utility  # noqa: E402


def link_ms(nbytes):
    """Milliseconds `nbytes` take host -> device from page-locked memory (best of three; the HIP runtime the library already
    loaded, through ctypes)."""
    import ctypes as C
    hip = C.CDLL("libamdhip64.so")
    host, dev = C.c_void_p(), C.c_void_p()
    if hip.hipHostMalloc(C.byref(host), C.c_size_t(nbytes), 0) != 0 or hip.hipMalloc(C.byref(dev), C.c_size_t(nbytes)) != 0:
        raise RuntimeError("hipHostMalloc / hipMalloc of %d bytes failed" % nbytes)
    try:
        C.memset(host, 1, nbytes)
        best = None
        for _ in range(3):
            hip.hipDeviceSynchronize()
            t0 = time.perf_counter()
            if hip.hipMemcpy(dev, host, C.c_size_t(nbytes), 1) != 0:        # 1: hipMemcpyHostToDevice
                raise RuntimeError("hipMemcpy failed")
            hip.hipDeviceSynchronize()
            dt = (time.perf_counter() - t0) * 1e3
            best = dt if best is None else min(best, dt)
        return best
    finally:
        hip.hipFree(dev)
        hip.hipHostFree(host)


def _mem_info():
    import ctypes as C
    hip = C.CDLL("libamdhip64.so")
    free, total = C.c_size_t(), C.c_size_t()
    if hip.hipMemGetInfo(C.byref(free), C.byref(total)) != 0:
        raise RuntimeError("hipMemGetInfo failed")
    return int(free.value), int(total.value)


def free_bytes():
    return _mem_info()[0]


def total_bytes():
    return _mem_info()[1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--configs', default='c2,c3')
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--dir', default='/dev/shm')
    ap.add_argument('--out', default=None)
    ap.add_argument('--commit', default='?', help="what is measured, for the output's first line")
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("tools/sam_e2e.py --configs %s --reps %d; commit %s; %s" % (a.configs, a.reps, a.commit, time.strftime("%Y-%m-%d")))

    root = tempfile.mkdtemp(prefix='sam_e2e_', dir=a.dir)
    try:
        with abi.Context(0) as ctx:
            info = ctx.device_info()
            say("device: %s" % info.get('name', '?'))
            for name in a.configs.split(','):
                cfg = dict(synth.CONFIGS[name])
                t0 = time.perf_counter()
                contigs, reads = synth.make_dataset(workers=min(16, utility.cpu_budget()), **cfg)
                refid = np.repeat(np.arange(contigs.n_contigs, dtype=np.int32), np.diff(contigs.read_begin))
                lens = [int(x) for x in contigs.length]
                sam, bam = os.path.join(root, name + '.sam'), os.path.join(root, name + '.bam')
                order = np.random.default_rng(1).permutation(reads.n_reads)
                synth.write_sam(sam, contigs.ids, lens, reads, refid, order=order)
                abi.write_bam(bam, contigs.ids, lens, refid, reads)
                text = os.path.getsize(sam)
                say("\n== %s: %d reads, %d contigs; genomes.sam %.1f MB (unsorted), genomes.bam %.1f MB; written in %.1f s"
                    % (name, reads.n_reads, contigs.n_contigs, text / 1e6, os.path.getsize(bam) / 1e6, time.perf_counter() - t0))
                thr = abi.Thresholds.from_args(abi.DEFAULT_ARGS)
                legs = {}
                for form, resident in (('columns', False), ('resident', True)):
                    # file -> batch ready -> first run, a.reps times; every handle and batch is released before the next rep
                    rows, best, best_ms = [], None, None
                    for rep in range(a.reps):
                        t0 = time.perf_counter()
                        decoded = abi.read_sam(sam, ctx, resident=resident)
                        t1 = time.perf_counter()
                        ms = abi.sam_decode_timing(ctx)
                        free_decoded = free_bytes()
                        assert isinstance(decoded[3], abi.ResidentReads) == resident
                        n = decoded[3].n_reads
                        batch = ctx.batch(contigs, decoded[3])
                        batch.sync()
                        t2 = time.perf_counter()
                        free_ready = free_bytes()
                        batch.run(thr)
                        batch.sync()
                        t3 = time.perf_counter()
                        path = abi.PATH_NAMES[batch.info().path]
                        batch.close()
                        del batch, decoded
                        rows.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, (t2 - t0) * 1e3, min(free_decoded, free_ready)))
                        if best is None or rows[-1][0] < best:
                            best, best_ms = rows[-1][0], ms
                        say("  %-8s rep %d: read_sam %8.1f ms, batch create %7.1f ms, first run (%s) %7.1f ms; file -> batch ready %8.1f ms; "
                            "free device memory, least seen %.2f GB (%d records)" % ((form, rep) + rows[-1][:2] + (path,) + rows[-1][2:4] + (rows[-1][4] / 1e9, n)))
                    say("  %s: the decode's phases (the rep with the fastest read_sam)" % form)
                    for k in abi.SAM_PHASES:
                        say("    %-18s %9.2f ms  %5.1f %%" % (k, best_ms[k], 100.0 * best_ms[k] / best))
                    rest = best - sum(best_ms.values())
                    say("    %-18s %9.2f ms  %5.1f %%  (device allocations and their release, unmapping, the binding)" % ('outside the phases', rest, 100.0 * rest / best))
                    cols = list(zip(*rows))
                    for label, v in zip(('read_sam', 'batch create', 'first run', 'file -> batch ready'), cols[:4]):
                        say("  %-8s %-20s median of %d: %8.1f ms  (min %.1f, max %.1f)" % (form, label, len(v), float(np.median(v)), min(v), max(v)))
                    say("  %-8s free device memory at the fullest moment a rep was looked at (decoded; batch ready): %.2f GB of %.2f GB"
                        % (form, min(cols[4]) / 1e9, total_bytes() / 1e9))
                    legs[form] = dict(ready=cols[3], best=best, ms=best_ms)
                c_med, r_med = float(np.median(legs['columns']['ready'])), float(np.median(legs['resident']['ready']))
                spread = max(legs['columns']['ready']) - min(legs['columns']['ready'])
                say("  file -> batch ready: columns %.1f ms, resident %.1f ms: resident is %.1f ms ahead; the column form's own min-max spread is %.1f ms -> %s"
                    % (c_med, r_med, c_med - r_med, spread, "beyond the spread" if c_med - r_med > spread else "inside the spread"))
                best, best_ms = legs['columns']['best'], legs['columns']['ms']
                say("  read_sam (columns) best: %.1f ms = %.2f GB/s of text" % (best, text / best / 1e6))
                bbest = None
                for rep in range(a.reps):
                    t0 = time.perf_counter()
                    decoded = abi.read_bam(bam, ctx, resident=True)
                    dt = (time.perf_counter() - t0) * 1e3
                    del decoded
                    bbest = dt if bbest is None else min(bbest, dt)
                say("  read_bam(resident=True) of the same reads, sorted: best %.1f ms  (SAM / BAM = %.2f)" % (bbest, best / bbest))
                link = link_ms(text)
                up2 = best_ms['upload'] + best_ms['pass 2 (payload)']
                say("  the link: %.1f MB from page-locked memory in %.1f ms (%.1f GB/s); upload + pass 2 = %.1f ms = %.2f x that"
                    % (text / 1e6, link, text / link / 1e6, up2, up2 / link))
                say("  pass 1 (a thread per line) is %.1f %% of the decode, the sort + gather %.1f %%"
                    % (100.0 * best_ms['pass 1 (fields)'] / best, 100.0 * best_ms['sort + gather'] / best))
                os.remove(sam)
                os.remove(bam)
    finally:
        shutil.rmtree(root, ignore_errors=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write("\n".join(lines) + "\n")


if __name__ == '__main__':
    main()
