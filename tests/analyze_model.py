"""A sequential Python model of Context.sites_scan (midas_sites_scan): the same arguments, the same outputs, every sum formed
the way the interpreter forms it.  The host tests inject it in place of the device (run_pipeline's make_context); the GPU tests
compare the device call with it bit for bit.  It is written from the reference's loop (midas/analyze/parse_snps.py,
scripts/snp_diversity.py, scripts/call_consensus.py), not from the kernels."""
import json
import os

import numpy as np

from midas_amd import abi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "analyze_vectors.json")


def load_vectors():
    with open(GOLDEN) as f:
        return json.load(f)


def pairwise_sum(a):
    """numpy's add.reduce of a list of floats: halves cut at multiples of eight down to blocks of at most 128, a block
    summed through eight partial sums."""
    n = len(a)
    if n < 8:
        res = 0.0
        for x in a:
            res += x
        return res
    if n <= 128:
        r = list(a[:8])
        i = 8
        while i < n - (n % 8):
            for j in range(8):
                r[j] += a[i + j]
            i += 8
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
        while i < n:
            res += a[i]
            i += 1
        return res
    n2 = n // 2
    n2 -= n2 % 8
    return pairwise_sum(a[:n2]) + pairwise_sum(a[n2:])


def pairwise_mean(a):
    return pairwise_sum(a) / len(a)


class BadCell(abi.MidasSnpsError):
    def __init__(self, bad, message):
        super().__init__(abi.ERR_BAD_LAYOUT, message)
        self.bad = bad


def _rows(text):
    """The rows of a matrix body as a text-mode csv.reader(delimiter='\\t') yields them (no quotes in these files)."""
    data = bytes(np.asarray(text, np.uint8)).decode('latin-1')
    lines = data.split('\n')
    if lines and lines[-1] == '':
        lines.pop()
    return [(ln[:-1] if ln.endswith('\r') else ln).split('\t') if ln != '' and ln != '\r' else [] for ln in lines]


def _py_max(a, b):
    return b if b > a else a


def _py_min(a, b):
    return b if b < a else a


def _py_round(x, i, s):
    """call_consensus: sample.freq = round(sample.freq), which raises on nan and inf."""
    try:
        return float(round(x))
    except (OverflowError, ValueError):
        raise BadCell((3, i, s), "data row %d, sample %d: the frequency to round is not a finite number" % (i, s))


def is_fast_float(cell):
    """Whether the device's own converter takes the cell: [+-]digits[.digits][e[+-]digits], mantissa < 2^53, |p10| <= 22."""
    import re
    m = re.fullmatch(r'[+-]?(\d+)(?:\.(\d+))?(?:[eE]([+-]?\d{1,3}))?', cell)
    if not m:
        return False
    mant = int(m.group(1) + (m.group(2) or ''))
    if mant >= 1 << 53:
        return False
    if mant == 0:
        return True
    e10 = int(m.group(3) or 0) - len(m.group(2) or '')
    return -22 <= e10 <= 22


def is_fast_int(cell):
    import re
    return re.fullmatch(r'[+-]?\d{1,18}', cell) is not None


def sites_scan(freq_text, depth_text, site_mask, sample_col, mean_depth, site_depth, site_ratio, allele_support, site_prev, site_maf,
               snp_maf=0.01, max_sites=-1, flags=0, site_gene=None, n_genes=0, minor=None, major=None, group_rows=0, chunk_bytes=0,
               dump=False, dump_keep=False):
    frows, drows = _rows(freq_text), _rows(depth_text)
    mask = np.asarray(site_mask, np.uint8)
    N = int(mask.shape[0])
    cols = [int(c) for c in sample_col]
    mean = [float(x) for x in mean_depth]
    S = len(cols)
    weight, rnd, pooled_mode = bool(flags & abi.SITES_WEIGHT), bool(flags & abi.SITES_ROUND), bool(flags & abi.SITES_POOLED)
    per_gene, mask_only = bool(flags & abi.SITES_PER_GENE), bool(flags & abi.SITES_MASK_ONLY)
    G = int(n_genes) if per_gene else 1
    chains = 1 if pooled_mode else S
    pi = [[0.0] * G for _ in range(chains)]
    snps = np.zeros((chains, G), np.int64)
    sites = np.zeros((chains, G), np.int64)
    depth = np.zeros((chains, G), np.int64)
    seq = [bytearray() for _ in range(S)]
    n = min(N, len(frows), len(drows))
    d_freq, d_depth = np.zeros((S, n)), np.zeros((S, n), np.int64)
    d_keep, d_pooled = np.zeros(n, np.uint8), np.zeros(n)
    side = [0, 0]
    kept = no_gene = 0
    n_read = 0
    for i in range(n):
        n_read = i + 1
        fr, dr = frows[i][1:], drows[i][1:]
        f, d = [], []
        for s in range(S):
            for m, (row, conv, fast, out) in enumerate(((fr, float, is_fast_float, f), (dr, int, is_fast_int, d))):
                if cols[s] >= len(row):
                    raise BadCell((m + 1, i, -1), "%s matrix, data row %d: fewer columns than the samples in use" % (('freq', 'depth')[m], i))
                cell = row[cols[s]]
                if not fast(cell):
                    side[m] += 1
                v = abi_parse(cell, m)
                if v is None:
                    raise BadCell((m + 1, i, s), "%s matrix, data row %d, sample %d: not a number" % (('freq', 'depth')[m], i, s))
                out.append(v)
        d_freq[:, i], d_depth[:, i] = f, d
        if max_sites >= 0 and kept >= max_sites:
            break
        keep = []
        for s in range(S):
            k = True
            if d[s] < site_depth:
                k = False
            if d[s] / mean[s] > site_ratio:
                k = False
            if _py_max(f[s], 1 - f[s]) < allele_support:
                k = False
            keep.append(k)
        f2 = [_py_round(x, i, s) if rnd else x for s, x in enumerate(f)]
        count = sum(keep)
        if count == 0:
            pooled = 0.0
        elif weight:
            dsum, msum = 0, 0.0
            for s in range(S):
                if keep[s]:
                    dsum += d[s]
                    msum += d[s] * f2[s]
            try:
                pooled = msum / dsum
            except ZeroDivisionError:
                raise BadCell((6, i, -1), "data row %d: the depths of the kept samples sum to 0, so no depth-weighted frequency" % i)
        else:
            pooled = pairwise_mean([f2[s] for s in range(S) if keep[s]])
        site_keep = bool(mask[i])
        if not mask_only:
            prev = float(count) / S
            if site_prev and prev < max(1e-6, site_prev):
                site_keep = False
            if site_maf and pooled < site_maf:
                site_keep = False
        d_pooled[i] = pooled
        if not site_keep:
            continue
        d_keep[i] = 1
        kept += 1
        g = int(site_gene[i]) if per_gene else 0
        if flags & abi.SITES_SUMS:
            if per_gene and g < 0:
                no_gene += 1
            elif pooled_mode:
                pi[0][g] += 2 * pooled * (1 - pooled)
                snps[0, g] += 1 if _py_min(pooled, 1 - pooled) >= snp_maf else 0
                sites[0, g] += 1
            else:
                for s in range(S):
                    if keep[s]:
                        pi[s][g] += 2 * f2[s] * (1 - f2[s])
                        snps[s, g] += 1 if _py_min(f2[s], 1 - f2[s]) >= snp_maf else 0
                        sites[s, g] += 1
                        depth[s, g] += d[s]
        if flags & abi.SITES_SEQ:
            for s in range(S):
                c = ord('-')
                if keep[s] and d[s] != 0:
                    c = int(minor[i]) if f[s] >= 0.5 else int(major[i])
                seq[s].append(c)
    out = dict(n_sites=n_read if (max_sites >= 0 and kept >= max_sites) else n, n_kept=kept, side_freq=side[0], side_depth=side[1],
               groups=1, no_gene=no_gene, ms=[0.0] * 8)
    if flags & abi.SITES_SUMS:
        out.update(pi=np.array(pi, np.float64).reshape(chains, G), snps=snps, sites=sites, depth=depth)
    if flags & abi.SITES_SEQ:
        out['seq'] = np.array([list(x) for x in seq], np.uint8).reshape(S, kept)
    if dump:
        out.update(freq=d_freq, depthv=d_depth, keep=d_keep, pooled=d_pooled)
    elif dump_keep:
        out['keep'] = d_keep
    return out


def abi_parse(cell, m):
    """float() / int() of a cell, or None -- Python's own."""
    try:
        return float(cell) if m == 0 else int(cell)
    except ValueError:
        return None


class ModelContext:
    """Stands in for abi.Context in the hosts' run_pipeline."""

    def sites_scan(self, *a, **kw):
        return sites_scan(*a, **kw)

    def close(self):
        pass
