"""Developer script (GPU box): `merge_midas.py snps` on one species, S samples x n sites, phase by phase -- through
midas_amd.merge.snps.merge_species alone, so that the same file runs on any commit that has it.

    python tools/merge_snps_e2e.py [--sites 2000000] [--samples 50] [--runs 5] [--modes device,host] [--readers host,device] [--data DIR] [--preset all_sites]

Setup (not timed): the samples' tables written with the library's own writer under --data (default: a fresh directory on tmpfs;
an existing one is reused, so two commits can be timed on the same files).  Timed: merge_species, --runs times per mode after one
warm-up, the modes taking turns (MIDAS_SNPS_MERGE_WRITERS=<mode>; a commit without the switch runs the host writers either way).
--readers: who reads the samples' tables (MIDAS_SNPS_MERGE_READERS=<reader>; default host): every reader x writer combination is
a mode of its own ("<reader> readers / <writer> writers").  'tables read' = load_sample_tables as a whole; the device readers' own
laps (upload, inflate + CRC, index, parse: HIP events) and counts are printed beside it.
Phases come from timers around the calls merge_species makes (tables read, the merge call, the host writers, snps_info) and,
where the library prints them (MIDAS_SNPS_TRACE), from its own `[merge tables]` line: upload, kernel, format, text down, file
write.  'tables out' = from the start of the merge call to the last byte of snps_freq / snps_depth: upload + kernel + (arrays or
text) down + format + file write -- the figure to compare between the writers.
"""
import argparse
import os
import re
import statistics
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from midas_amd import abi, synth  # noqa: E402
from midas_amd.merge import annotate, merge, snps as msnps  # noqa: E402


def make_data(root, n, S):
    rng = np.random.default_rng(0)
    n_contigs = 60
    lens = [n // n_contigs] * n_contigs
    lens[-1] += n - sum(lens)
    ids = sorted("sp1_c%03d" % k for k in range(n_contigs))
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    ref_idx = rng.integers(0, 4, n)
    ref = letters[ref_idx]
    db = os.path.join(root, "db")
    for d in ("marker_genes", "pan_genomes", "rep_genomes/sp1"):
        os.makedirs(os.path.join(db, d), exist_ok=True)
    synth.write_db_tables(db, ["sp1"])
    off = np.concatenate([[0], np.cumsum(lens)])
    with open(os.path.join(db, "rep_genomes/sp1/genome.fna"), "w") as h:
        for k, cid in enumerate(ids):
            h.write(">%s\n%s\n" % (cid, ref[off[k]:off[k + 1]].tobytes().decode()))
    synth.write_features(db, "sp1", synth.make_genes(rng, ids, lens))
    alt = (ref_idx + rng.integers(1, 4, n)) % 4
    snp = rng.random(n) < 0.03
    for s in range(S):
        depth = rng.poisson(10.0, n).astype(np.uint32)
        na = np.where(snp, rng.binomial(depth, 0.3), 0).astype(np.uint32)
        c = np.zeros((n, 4), np.uint32)
        c[np.arange(n), ref_idx] = depth - na
        c[np.arange(n), alt] += na
        sdir = os.path.join(root, "samples", "s%02d" % s)
        os.makedirs(os.path.join(sdir, "snps", "output"), exist_ok=True)
        abi.write_table(os.path.join(sdir, "snps", "output", "sp1.snps.gz"), ids, [ref[off[k]:off[k + 1]] for k in range(n_contigs)],
                        [c[off[k]:off[k + 1]] for k in range(n_contigs)], threads=0)
        tot = c.sum(1)
        cov = int((tot > 0).sum())
        with open(os.path.join(sdir, "snps", "summary.txt"), "w") as h:
            h.write("species_id\tgenome_length\tcovered_bases\tfraction_covered\tmean_coverage\taligned_reads\tmapped_reads\n")
            h.write("sp1\t%d\t%d\t%s\t%s\t%d\t%d\n" % (n, cov, cov / float(n), float(tot.sum()) / cov, 1000, 900))
    with open(os.path.join(root, "shape.txt"), "w") as h:
        h.write("%d %d\n" % (n, S))


class Timers:
    """Wall time of the calls merge_species makes, by name; 'first' / 'last' of the merge call and the writers for 'tables out'."""
    def __init__(self):
        self.t = {}
        self.span = {}

    def wrap(self, owner, name, label):
        if not hasattr(owner, name):
            return
        f = getattr(owner, name)

        def g(*a, **k):
            t0 = time.perf_counter()
            try:
                return f(*a, **k)
            finally:
                t1 = time.perf_counter()
                self.t[label] = self.t.get(label, 0.0) + t1 - t0
                lo, hi = self.span.get(label, (t0, t1))
                self.span[label] = (min(lo, t0), max(hi, t1))
        setattr(owner, name, g)

    def reset(self):
        self.t, self.span = {}, {}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sites", type=int, default=2_000_000)
    ap.add_argument("--samples", type=int, default=50)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--modes", default="device,host")
    ap.add_argument("--readers", default="host")
    ap.add_argument("--data", default=None)
    ap.add_argument("--preset", default="all_sites", choices=["all_sites", "core_snps"])
    ap.add_argument("--threads", type=int, default=16)
    a = ap.parse_args()
    tmpfs = "/dev/shm" if os.path.isdir("/dev/shm") else None
    root = a.data or tempfile.mkdtemp(prefix="merge_snps_e2e_", dir=tmpfs)
    t0 = time.time()
    if not os.path.exists(os.path.join(root, "shape.txt")):
        os.makedirs(root, exist_ok=True)
        make_data(root, a.sites, a.samples)
    n, S = [int(x) for x in open(os.path.join(root, "shape.txt")).read().split()]
    print("setup (not part of the command): %.1f s; %d sites x %d samples under %s" % (time.time() - t0, n, S, root), flush=True)
    samples = sorted(os.path.join(root, "samples", d) for d in os.listdir(os.path.join(root, "samples")))
    out = tempfile.mkdtemp(prefix="out_", dir=root)
    args = dict(outdir=out, db=os.path.join(root, "db"), indirs=samples, species_id=None, max_samples=None, sample_depth=5.0,
                fract_cov=0.4, min_samples=1, max_species=None, threads=a.threads, max_sites=float('Inf'), **abi.DEFAULT_MERGE_ARGS)
    if a.preset == 'all_sites':
        args.update(snp_type=['any'], site_prev=0.0)
    sp = merge.select_species(args, 'snps')[0]
    T = Timers()
    T.wrap(msnps, 'load_sample_tables', 'tables read')
    T.wrap(abi, 'read_snps_counts', 'tables read: the host readers of samples 1..S-1')
    T.wrap(abi, 'read_snps_table', 'tables read (first sample, beside the others)')
    T.wrap(abi, 'write_merge_matrix', 'host writers')
    T.wrap(abi, 'write_merge_info', 'info')
    T.wrap(annotate.GeneCursor, 'from_db', 'gene table (beside the tables read)')
    T.wrap(abi.Context, 'merge_sites', 'merge call')
    T.wrap(abi.Context, 'merge_sites_tables', 'merge call')
    device_laps = []
    if hasattr(abi.Context, 'read_snps_counts_device'):
        read_on_device = abi.Context.read_snps_counts_device

        def timed_read(self, *args_, **kw):
            t0 = time.perf_counter()
            tables = read_on_device(self, *args_, **kw)
            device_laps.append(dict(tables.ms, **{'whole call (open + plan + laps)': (time.perf_counter() - t0) * 1e3}, **{k: float(v) for k, v in tables.stats.items()}))
            return tables
        abi.Context.read_snps_counts_device = timed_read
    ctx = abi.Context(0)
    modes = ["%s/%s" % (r, w) for r in a.readers.split(",") for w in a.modes.split(",")]
    laps = {m: [] for m in modes}
    os.environ['MIDAS_SNPS_TRACE'] = '1'
    trace_path = os.path.join(root, "trace.txt")
    rows = {m: [] for m in modes}
    traces = {m: [] for m in modes}
    kept = None
    for it in range(a.runs + 1):          # run 0 warms up (page cache, pinned ring, device buffers)
        for m in modes:
            os.environ['MIDAS_SNPS_MERGE_READERS'], os.environ['MIDAS_SNPS_MERGE_WRITERS'] = m.split("/")
            T.reset()
            del device_laps[:]
            sys.stderr.flush()
            saved = os.dup(2)
            fd = os.open(trace_path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC)
            os.dup2(fd, 2)
            try:
                t_start = time.perf_counter()
                nn, kept, kms = msnps.merge_species(sp, args, ctx)
                total = time.perf_counter() - t_start
            finally:
                os.dup2(saved, 2)
                os.close(fd)
                os.close(saved)
            begin = T.span['merge call'][0]
            end = T.span.get('host writers', T.span['merge call'])[1]
            r = dict(T.t)
            r['tables out'] = end - begin
            r['whole merge_species'] = total
            r['kernel ms'] = kms
            line = [l for l in open(trace_path).read().splitlines() if l.startswith('[merge tables]')]
            if it > 0:
                rows[m].append(r)
                if line:
                    traces[m].append(line[-1])
                laps[m].extend(device_laps)
            sizes = [os.path.getsize(os.path.join(out, 'sp1', f)) for f in ('snps_freq.txt', 'snps_depth.txt', 'snps_info.txt')]
            print("  run %d %-13s tables out %.3f s, whole %.3f s (freq %d B, depth %d B, info %d B)%s"
                  % (it, m, r['tables out'], total, sizes[0], sizes[1], sizes[2], "  [warm-up]" if it == 0 else ""), flush=True)
    print("\n%d sites x %d samples, %d kept rows, preset %s, %d runs a mode after one warm-up; median [min .. max], seconds" % (n, S, kept, a.preset, a.runs))
    for m in modes:
        print("mode %s readers / %s writers" % tuple(m.split("/")))
        for k in sorted(rows[m][0]):
            v = [r.get(k, 0.0) for r in rows[m]]
            print("  %-48s %9.4f  [%9.4f .. %9.4f]" % (k, statistics.median(v), min(v), max(v)))
        if laps[m]:
            for key in laps[m][0]:
                v = [l[key] for l in laps[m]]
                print("  device readers: %-32s %12.3f  [%12.3f .. %12.3f]%s" % (key, statistics.median(v), min(v), max(v), "  ms" if key in abi.TABLES_READ_PHASES or 'call' in key else ""))
        if traces[m]:
            nums = {}
            for l in traces[m]:
                for key, pat in (('upload s', r'upload ([\d.]+) s'), ('kernel ms', r'kernel ([\d.]+) ms'), ('per-site results down s', r'results down ([\d.]+) s'),
                                 ('rows s (format + text down + waits for the writer)', r'rows ([\d.]+) s'), ('format ms (device)', r'format ([\d.]+) ms'),
                                 ('text down s', r'text down ([\d.]+) s'), ('file write s (writer thread)', r'file write ([\d.]+) s'),
                                 ('file write after the last batch s', r'\(([\d.]+) s of it after'), ('text bytes', r'(\d+) bytes of text')):
                    mm = re.search(pat, l)
                    if mm:
                        nums.setdefault(key, []).append(float(mm.group(1)))
            for key, v in nums.items():
                print("  library: %-39s %12.4f  [%12.4f .. %12.4f]" % (key, statistics.median(v), min(v), max(v)))
            if 'text bytes' in nums and 'format ms (device)' in nums:
                text = statistics.median(nums['text bytes'])
                fms = statistics.median(nums['format ms (device)'])
                # the formatter reads 8 B a cell for the freq table and 4 B a cell for the depth table in each of its two passes
                cells = float(kept) * S
                print("  link: %.0f MB of text + %.0f MB of per-site results down (host writers: %.0f MB of arrays + the same results)"
                      % (text / 1e6, n * 40 / 1e6, 2.0 * S * n * 4 / 1e6))
                need = cells * 8 + text
                print("  formatter: must read %.0f MB (8 B a cell) and write %.0f MB of text; %.3f ms on the device = %.1f GB/s = %.1f %% of the 8 TB/s HBM peak"
                      % (cells * 8 / 1e6, text / 1e6, fms, need / fms / 1e6, 100.0 * need / (fms * 1e-3) / 8e12))
    if len(modes) == 2 and len(a.readers.split(",")) == 1:
        a0, a1 = ([r['tables out'] for r in rows[m]] for m in modes)
        print("tables out, %s vs %s: medians %.3f vs %.3f s; spread (max - min) %.3f and %.3f s" %
              (modes[0], modes[1], statistics.median(a0), statistics.median(a1), max(a0) - min(a0), max(a1) - min(a1)))
    if len(a.readers.split(",")) == 2:
        for w in a.modes.split(","):
            r0, r1 = ("%s/%s" % (r, w) for r in a.readers.split(","))
            for key in ('tables read', 'whole merge_species'):
                v0, v1 = [r[key] for r in rows[r0]], [r[key] for r in rows[r1]]
                print("%s, %s writers, %s vs %s readers: medians %.3f vs %.3f s; spread (max - min) %.3f and %.3f s" %
                      (key, w, r0.split("/")[0], r1.split("/")[0], statistics.median(v0), statistics.median(v1), max(v0) - min(v0), max(v1) - min(v1)))
    ctx.close()


if __name__ == "__main__":
    main()
