"""A sequential model of Context.sites_pair_diversity (midas_sites_pair_diversity) in plain Python, written from the two contracts
of midas_amd/analyze/pairs.py and from the reference's loop (GenomicSite.flag_samples, compute_pooled_maf, filter; the pooled
branch of compute_snp_diversity), not from the kernel: one pair after the other, one site after the other, every sum one
interpreter operation a term.  Rows come from analyze_model's reader, min / max / round are its Python-rule helpers.  The host
tests inject ModelContext in place of the device; the GPU tests compare the device call with the model bit for bit."""
import numpy as np

from midas_amd import abi
from tests import analyze_model as M
from tests import snp_trees_model

KEYS_INT, KEYS_F64 = ('sites', 'snps', 'shared'), ('pi', 'w1', 'w2', 'x')


def read_cells(freq_text, depth_text, n_mask, sample_col, round_freq):
    """-> (f [n][S] floats as read, the same rounded under round_freq, d [n][S] ints): row by row, sample by sample, the frequency before the depth,
    then the row's frequencies are rounded -- the first cell the reference cannot convert or round is the error."""
    frows, drows = M._rows(freq_text), M._rows(depth_text)
    n = min(n_mask, len(frows), len(drows))
    cols = [int(c) for c in sample_col]
    raw, fs, ds = [], [], []
    for i in range(n):
        fr, dr = frows[i][1:], drows[i][1:]
        f, d = [], []
        for s, c in enumerate(cols):
            for m, (row, out) in enumerate(((fr, f), (dr, d))):
                if c >= len(row):
                    raise M.BadCell((m + 1, i, -1), "%s matrix, data row %d: fewer columns than the samples in use" % (('freq', 'depth')[m], i))
                v = M.abi_parse(row[c], m)
                if v is None:
                    raise M.BadCell((m + 1, i, s), "%s matrix, data row %d, sample %d: not a number" % (('freq', 'depth')[m], i, s))
                out.append(v)
        raw.append(f)
        fs.append([M._py_round(x, i, s) for s, x in enumerate(f)] if round_freq else f)
        ds.append(d)
    return raw, fs, ds


def flag_cells(fs_raw, ds, mean, site_depth, site_ratio, allele_support):
    """GenomicSite.flag_samples over the unrounded frequencies -> keep [n][S]."""
    keep = []
    for f, d in zip(fs_raw, ds):
        row = []
        for s in range(len(mean)):
            k = True
            if d[s] < site_depth:
                k = False
            if d[s] / mean[s] > site_ratio:
                k = False
            if M._py_max(f[s], 1 - f[s]) < allele_support:
                k = False
            row.append(k)
        keep.append(row)
    return keep


def pooled_of_pair(a, b, da, db, ka, kb, weight):
    """compute_pooled_maf over the two cells, i before j."""
    count = int(ka) + int(kb)
    if count == 0:
        return 0.0, 0
    if weight:
        dsum, msum = 0, 0.0
        if ka:
            dsum += da
            msum += da * a
        if kb:
            dsum += db
            msum += db * b
        return msum / dsum, count
    total = 0.0                   # (numpy's add.reduce of fewer than eight values: from 0.0, left to right)
    if ka:
        total += a
    if kb:
        total += b
    return total / count, count


def one_pair(fs, ds, keep, mask, i, j, weight, site_prev, site_maf, snp_maf, max_sites):
    """Both contracts for the pair (i, j) -> dict(sites, snps, shared, pi, w1, w2, x, rows: the rows it retained)."""
    sites = snps = shared = 0
    pi = w1 = w2 = x = 0.0
    rows = []
    for r in range(len(fs)):
        if not mask[r]:
            continue
        a, b, ka, kb = fs[r][i], fs[r][j], keep[r][i], keep[r][j]
        p, count = pooled_of_pair(a, b, ds[r][i], ds[r][j], ka, kb, weight)
        if site_prev and float(count) / 2 < max(1e-6, site_prev):
            continue
        if site_maf and p < site_maf:
            continue
        if max_sites >= 0 and sites >= max_sites:
            continue
        rows.append(r)
        sites += 1
        pi += (2.0 * p) * (1.0 - p)
        snps += 1 if M._py_min(p, 1 - p) >= snp_maf else 0
        if ka and kb:
            shared += 1
            w1 += (2.0 * a) * (1.0 - a)
            w2 += (2.0 * b) * (1.0 - b)
            x += (a * (1.0 - b)) + (b * (1.0 - a))
    return dict(sites=sites, snps=snps, shared=shared, pi=pi, w1=w1, w2=w2, x=x, rows=rows)


def sites_pair_diversity(freq_text, depth_text, site_mask, sample_col, mean_depth, site_depth, site_ratio, allele_support, site_prev,
                         site_maf, snp_maf=0.01, max_sites=-1, flags=0, group_rows=0, chunk_bytes=0, pair_form=0, _rows_out=None):
    mask = np.asarray(site_mask, np.uint8)
    S = len(sample_col)
    weight, rnd = bool(flags & abi.SITES_WEIGHT), bool(flags & abi.SITES_ROUND)
    if S < 2 or group_rows < 0 or chunk_bytes < 0 or pair_form not in (0, 1, 2) or (weight and site_depth < 1):
        raise abi.MidasSnpsError(abi.ERR_INVALID_ARG, "invalid argument")
    mean = [float(v) for v in mean_depth]
    fs_raw, fs, ds = read_cells(freq_text, depth_text, int(mask.shape[0]), sample_col, rnd)
    keep = flag_cells(fs_raw, ds, mean, site_depth, site_ratio, allele_support)
    out = {k: np.zeros((S, S), np.int64) for k in KEYS_INT}
    out.update({k: np.zeros((S, S), np.float64) for k in KEYS_F64})
    for i in range(S):
        for j in range(i + 1, S):
            one = one_pair(fs, ds, keep, mask, i, j, weight, site_prev, site_maf, snp_maf, max_sites)
            for k in KEYS_INT + KEYS_F64:
                out[k][i, j] = one[k]
            if _rows_out is not None:
                _rows_out[(i, j)] = one['rows']
    out.update(n_sites=len(fs), n_masked=int(np.count_nonzero(mask[:len(fs)])), groups=1, ms=[0.0] * 8)
    return out


class ModelContext(M.ModelContext):
    """Stands in for abi.Context in pairs.run_pipeline (and, through analyze_model's sites_scan, in diversity.run_pipeline)."""

    def sites_pair_diversity(self, *a, **kw):
        return sites_pair_diversity(*a, **kw)

    def nj_tree(self, dist):
        return snp_trees_model.nj_tree(dist)
