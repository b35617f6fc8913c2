"""Writes tests/golden/assoc_vectors.json: what scipy gives for the p-values, ranks and q-values of gene_assoc.py (DESIGN.md section
22).  Run on a CPU with scipy (1.15.3 wrote the committed file): python tests/golden/make_assoc_vectors.py

  fisher    (a, c, n1, n2) with scipy.stats.fisher_exact's two-sided p
  ranksum   value / label vectors with scipy.stats.rankdata's midranks, scipy.stats.mannwhitneyu's p (asymptotic, continuity
            correction) and its U1; heavy ties, all-equal values and group sizes from 1 + 1 to 400 + 600 among them.  A vector
            is kept short: its distinct values ascending (levels), the level of every sample (index; a string of digits where there are at most ten levels), the labels as a string
            of 0 / 1, and scipy's doubled midrank of every level (ranks2)
  bh        p-value vectors with scipy.stats.false_discovery_control(method='bh')
The file holds data only.  worst_rel_diff records the largest relative difference seen here between the contract's expression
(tests/gene_assoc_model.py) and scipy's value, per kind; it must stay below 1e-9 (a larger one means the formula is wrong); the
test allows ten times the recorded value, for another machine's lgamma / exp / erfc.
"""
import json
import os
import sys

import numpy as np
import scipy
import scipy.stats

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import gene_assoc_model as M      # noqa: E402


def rel(a, b):
    return 0.0 if a == b else abs(a - b) / max(abs(a), abs(b))


def main():
    rng = np.random.default_rng(20261021)
    worst = dict(fisher=0.0, ranksum=0.0, bh=0.0)
    fisher = []
    sizes = [(1, 1), (1, 5), (3, 4), (4, 3), (7, 7), (10, 30), (25, 25), (60, 40), (150, 50), (400, 600)]
    for n1, n2 in sizes:
        N = n1 + n2
        for _ in range(20):
            c = int(rng.integers(0, N + 1))
            lo, hi = max(0, c - n2), min(n1, c)
            a = int(rng.integers(lo, hi + 1))
            p = float(scipy.stats.fisher_exact([[a, c - a], [n1 - a, n2 - (c - a)]], alternative='two-sided')[1])
            worst['fisher'] = max(worst['fisher'], rel(M.fisher(a, c, n1, n2), p))
            fisher.append([a, c, n1, n2, p])
    ranksum = []
    for n1, n2 in sizes:
        N = n1 + n2
        for kind in ('distinct', 'few values', 'mostly zero', 'all equal'):
            if kind == 'distinct' and N > 100:
                continue                                # (a level a sample: nothing to keep short)
            if kind == 'distinct':
                v = rng.permutation(N).astype(np.float64) * 0.25
            elif kind == 'few values':
                v = rng.integers(0, 4, N).astype(np.float64) * 0.5
            elif kind == 'mostly zero':
                v = np.where(rng.random(N) < 0.8, 0.0, np.round(rng.random(N) * 3, 1))
            else:
                v = np.full(N, 1.25)
            label = np.zeros(N, np.int64)
            label[rng.permutation(N)[:n1]] = 1
            ranks = scipy.stats.rankdata(v, method='average')
            r2, T = M.midranks(v)
            assert np.array_equal(r2, (2 * ranks).astype(np.int64)) and np.array_equal(2 * ranks, np.round(2 * ranks))
            counts = np.unique(v, return_counts=True)[1].astype(np.int64)
            assert T == int((counts ** 3 - counts).sum())
            levels, index = np.unique(v, return_inverse=True)
            first = [int(np.flatnonzero(index == k)[0]) for k in range(levels.shape[0])]
            assert all((r2[index == k] == r2[first[k]]).all() for k in range(levels.shape[0]))
            rec = dict(levels=levels.tolist(), index=''.join(str(k) for k in index) if levels.shape[0] <= 10 else index.tolist(), label=''.join(str(x) for x in label.tolist()),
                       ranks2=[int(r2[k]) for k in first], ties=T, p=None, U1=None)
            if kind != 'all equal':
                res = scipy.stats.mannwhitneyu(v[label == 1], v[label == 0], use_continuity=True, alternative='two-sided', method='asymptotic')
                U1, p = M.ranksum(int(r2[label == 1].sum()), T, n1, n2)
                assert U1 == float(res.statistic)
                worst['ranksum'] = max(worst['ranksum'], rel(p, float(res.pvalue)))
                rec['p'], rec['U1'] = float(res.pvalue), float(res.statistic)
            ranksum.append(rec)
    bh = []
    for m in (1, 2, 5, 17, 40):
        for kind in range(3):
            p = np.maximum(np.round(rng.random(m) ** (kind + 1), 5), 1e-5)
            if kind == 2:
                p = np.round(p, 2)                      # ties among the p-values
                p[p == 0] = 0.01
            q = scipy.stats.false_discovery_control(p, method='bh')
            worst['bh'] = max([worst['bh']] + [rel(x, float(y)) for x, y in zip(M.bh(p.tolist()), q)])
            bh.append(dict(p=p.tolist(), q=[float(x) for x in q]))
    assert max(worst.values()) < 1e-9, worst
    out = dict(scipy=scipy.__version__, worst_rel_diff=worst, fisher=fisher, ranksum=ranksum, bh=bh)
    with open(os.path.join(HERE, 'assoc_vectors.json'), 'w') as f:
        f.write('{\n' + ',\n'.join('%s:%s' % (json.dumps(k), json.dumps(v, separators=(',', ':'))) for k, v in out.items()) + '\n}\n')
    print(worst, len(fisher), len(ranksum), len(bh))


if __name__ == '__main__':
    main()
