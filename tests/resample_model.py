"""A sequential Python model of Context.sites_scan with rand_reads (midas_sites_scan_resampled): analyze_model's site loop with
GenomicSite.resample_reads and the second compute_pooled_maf in their place, written from the semantics -- not from the kernels
and not from the reference's text.  The draws are restated on the raw MT19937 stream: np.random.choice(list of N, N) is
randint(0, N, N), which takes one 32-bit word a try, ANDs it with the smallest 2^k - 1 >= N - 1 and keeps the value when it is
<= N - 1; N = 1 takes nothing.  The host tests hold this restatement to np.random.choice itself and to the reference's own
output (tests/golden/resample_vectors.json); the GPU tests compare the device call with sites_scan() bit for bit."""
import json
import os

import numpy as np

from midas_amd import abi
from tests import analyze_model as A

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resample_vectors.json")


def load_vectors():
    with open(GOLDEN) as f:
        return json.load(f)


def draw_mask(n):
    m = n - 1
    for k in (1, 2, 4, 8, 16):
        m |= m >> k
    return m


def legacy_state(key, pos):
    return ('MT19937', np.asarray(key, np.uint32), int(pos), 0, 0.0)


class RawStream:
    """numpy's legacy generator from a get_state() value, one raw 32-bit word at a time; consumed counts them."""

    def __init__(self, state):
        self.key, self.pos = np.array(state[1], np.uint32), int(state[2])
        self._bg = self._at_start()
        self._words, self.consumed = [], 0

    def _at_start(self):
        bg = np.random.MT19937()
        bg.state = dict(bit_generator='MT19937', state=dict(key=self.key.copy(), pos=self.pos))
        return bg

    def word(self):
        if self.consumed == len(self._words):
            self._words.extend(int(w) for w in self._bg.random_raw(4096))
        self.consumed += 1
        return self._words[self.consumed - 1]

    def accepted(self, n):
        """one value of randint(0, n): tries until a masked word is <= n - 1"""
        mask = draw_mask(n)
        while True:
            v = self.word() & mask
            if v <= n - 1:
                return v

    def state(self):
        """the legacy state behind the last word taken"""
        bg = self._at_start()
        if self.consumed:
            bg.random_raw(self.consumed)
        st = bg.state['state']
        return legacy_state(st['key'], st['pos'])


def resample_cell(f, n, replace, stream):
    """-> the minor reads k of a cell with 0 < f < 1: count_minor = round(f * n), half to even; without replacement all n reads are
    picked, so k = count_minor; with replacement k of the n draws fall below count_minor (the list is [1] * count_minor + [0] * rest)."""
    count_minor = int(round(f * n))
    if not replace or n == 1:
        return count_minor
    return sum(1 for _ in range(n) if stream.accepted(n) < count_minor)


def sites_scan(freq_text, depth_text, site_mask, sample_col, mean_depth, site_depth, site_ratio, allele_support, site_prev, site_maf,
               snp_maf=0.01, max_sites=-1, flags=0, site_gene=None, n_genes=0, minor=None, major=None, group_rows=0, chunk_bytes=0,
               dump=False, dump_keep=False, rand_reads=0, replace_reads=False, np_state=None, draw_chunk=0):
    if not rand_reads:
        return A.sites_scan(freq_text, depth_text, site_mask, sample_col, mean_depth, site_depth, site_ratio, allele_support, site_prev,
                            site_maf, snp_maf, max_sites, flags, site_gene, n_genes, minor, major, group_rows, chunk_bytes, dump, dump_keep)
    if flags & abi.SITES_SEQ or rand_reads < 0:
        raise abi.MidasSnpsError(abi.ERR_INVALID_ARG, "rand_reads")
    N = int(rand_reads)
    state = np_state if np_state is not None else np.random.get_state()
    stream = RawStream(state)
    frows, drows = A._rows(freq_text), A._rows(depth_text)
    mask = np.asarray(site_mask, np.uint8)
    cols = [int(c) for c in sample_col]
    mean = [float(x) for x in mean_depth]
    S = len(cols)
    weight, rnd, pooled_mode = bool(flags & abi.SITES_WEIGHT), bool(flags & abi.SITES_ROUND), bool(flags & abi.SITES_POOLED)
    per_gene, mask_only = bool(flags & abi.SITES_PER_GENE), bool(flags & abi.SITES_MASK_ONLY)
    G = int(n_genes) if per_gene else 1
    chains = 1 if pooled_mode else S
    pi = [[0.0] * G for _ in range(chains)]
    snps, sites, depth = (np.zeros((chains, G), np.int64) for _ in range(3))
    n = min(int(mask.shape[0]), len(frows), len(drows))
    d_freq, d_depth = np.zeros((S, n)), np.zeros((S, n), np.int64)
    d_keep, d_pooled = np.zeros(n, np.uint8), np.zeros(n)
    side = [0, 0]
    kept = no_gene = n_read = n_resampled = n_drew = 0

    def pool(f2, d, keep):
        count = sum(keep)
        if count == 0:
            return 0.0
        if weight:
            dsum, msum = 0, 0.0
            for s in range(S):
                if keep[s]:
                    dsum += d[s]
                    msum += d[s] * f2[s]
            return msum / dsum
        return A.pairwise_mean([f2[s] for s in range(S) if keep[s]])

    for i in range(n):
        n_read = i + 1
        fr, dr = frows[i][1:], drows[i][1:]
        f, d = [], []
        for s in range(S):
            for m, (row, fast, out) in enumerate(((fr, A.is_fast_float, f), (dr, A.is_fast_int, d))):
                if cols[s] >= len(row):
                    raise A.BadCell((m + 1, i, -1), "%s matrix, data row %d: fewer columns than the samples in use" % (('freq', 'depth')[m], i))
                cell = row[cols[s]]
                side[m] += not fast(cell)
                v = A.abi_parse(cell, m)
                if v is None:
                    raise A.BadCell((m + 1, i, s), "%s matrix, data row %d, sample %d: not a number" % (('freq', 'depth')[m], i, s))
                out.append(v)
        d_freq[:, i], d_depth[:, i] = f, d
        if max_sites >= 0 and kept >= max_sites:
            break
        keep = [not (d[s] < site_depth or d[s] / mean[s] > site_ratio or A._py_max(f[s], 1 - f[s]) < allele_support) for s in range(S)]
        f2 = [A._py_round(x, i, s) if rnd else x for s, x in enumerate(f)]
        if weight and sum(keep) and sum(d[s] for s in range(S) if keep[s]) == 0:
            raise A.BadCell((6, i, -1), "data row %d: the depths of the kept samples sum to 0, so no depth-weighted frequency" % i)
        pooled = pool(f2, d, keep)
        site_keep = bool(mask[i])
        if not mask_only:
            if site_prev and float(sum(keep)) / S < max(1e-6, site_prev):
                site_keep = False
            if site_maf and pooled < site_maf:
                site_keep = False
        d_pooled[i] = pooled
        if not site_keep:
            continue
        d_keep[i] = 1
        kept += 1
        if pooled > 0.0:                        # resample_reads: every selected sample, kept or not; then the pooled frequency again
            n_resampled += 1
            for s in range(S):
                d[s] = N
                if 0 < f2[s] < 1:
                    n_drew += 1
                    f2[s] = resample_cell(f2[s], N, replace_reads, stream) / N
                    f[s] = f2[s]
            pooled = pool(f2, d, keep)
            d_freq[:, i], d_depth[:, i], d_pooled[i] = f, d, pooled
        g = int(site_gene[i]) if per_gene else 0
        if flags & abi.SITES_SUMS:
            if per_gene and g < 0:
                no_gene += 1
            elif pooled_mode:
                pi[0][g] += 2 * pooled * (1 - pooled)
                snps[0, g] += 1 if A._py_min(pooled, 1 - pooled) >= snp_maf else 0
                sites[0, g] += 1
            else:
                for s in range(S):
                    if keep[s]:
                        pi[s][g] += 2 * f2[s] * (1 - f2[s])
                        snps[s, g] += 1 if A._py_min(f2[s], 1 - f2[s]) >= snp_maf else 0
                        sites[s, g] += 1
                        depth[s, g] += d[s]
    out = dict(n_sites=n_read if (max_sites >= 0 and kept >= max_sites) else n, n_kept=kept, side_freq=side[0], side_depth=side[1],
               groups=1, no_gene=no_gene, ms=[0.0] * 8, n_resampled=n_resampled, n_drew=n_drew, raw_consumed=stream.consumed,
               np_state=stream.state() if stream.consumed else legacy_state(state[1], state[2]))
    if flags & abi.SITES_SUMS:
        out.update(pi=np.array(pi, np.float64).reshape(chains, G), snps=snps, sites=sites, depth=depth)
    if dump:
        out.update(freq=d_freq, depthv=d_depth, keep=d_keep, pooled=d_pooled)
    elif dump_keep:
        out['keep'] = d_keep
    return out


class ModelContext(A.ModelContext):
    """analyze_model's double of the device, with rand_reads."""

    def sites_scan(self, *a, **kw):
        return sites_scan(*a, **kw)


def end_key(case):
    """the 624 key words numpy's generator held when the reference's loop ended"""
    import base64
    return np.frombuffer(base64.b64decode(case['end_key']), '<u4')


def write_tree(tmp, vec):
    """the golden species as directories under tmp"""
    for name, sp in vec['species'].items():
        d = '%s/%s' % (tmp, name)
        os.makedirs(d, exist_ok=True)
        for k in ('summary', 'info', 'freq', 'depth'):
            with open('%s/snps_%s.txt' % (d, k), 'w', newline='') as f:
                f.write(sp[k])
    return tmp


def run_case(tree, case, out, make_context=ModelContext, extra=()):
    """One golden case through the command's own layers, both global streams seeded as the maker seeded them.
    -> (run_pipeline's result, numpy's legacy state afterwards)."""
    import contextlib
    import io
    import random
    from midas_amd.analyze import cli, diversity
    args = cli.diversity_arguments(['%s/%s' % (tree, case['species'])] + list(case['options']) + list(extra) + ['--out', out])
    cli.check_diversity_args(args, resampling=True)
    np.random.seed(case['seed'])
    random.seed(case['seed'])
    with contextlib.redirect_stdout(io.StringIO()):
        res = diversity.run_pipeline(args, make_context=make_context)
    return res, np.random.get_state()


def check_case(tree, case, out, make_context=ModelContext, extra=()):
    """The output is the reference's, byte for byte (per-gene rows in any order: the reference walks a set), and numpy's global
    stream stands where the reference's loop left it -- with replacement; without, where the loop found it."""
    res, after = run_case(tree, case, out, make_context, extra)
    per_gene = 'per-gene' in case['options']
    rows = lambda text: [text.split('\n')[0]] + sorted(text.split('\n')[1:]) if per_gene else text.split('\n')
    assert rows(open(out).read()) == rows(case['out'])
    if '--replace_reads' in case['options']:
        assert int(after[2]) == case['end_pos'] and np.array_equal(after[1], end_key(case))
        assert res['raw_consumed'] == case['raw_words']
    else:
        assert res['raw_consumed'] == 0
        assert int(after[2]) == int(res['np_state'][2]) and np.array_equal(after[1], res['np_state'][1])
    return res
