"""A sequential model of snp_trees.py: the consensus planes and pair counts out of analyze_model.sites_scan's sequences, the
division, neighbour joining exactly as include/midas_snps.h writes it, in fp64 one operation at a time, and the two writers.
The host tests inject ModelContext in place of the device; the GPU tests compare the device calls and the script's files with it.
Also here: random additive trees, the oracle the model itself is held to."""
import os

import numpy as np

from midas_amd import abi
from midas_amd.analyze import cli, sites, trees
from tests import analyze_model

MINOR, MAJOR = 1, 2             # the allele bytes handed to sites_scan: the sequences then spell the allele's role


def sites_consensus_pairs(freq_text, depth_text, site_mask, sample_col, mean_depth, site_depth, site_ratio, allele_support, site_prev,
                          site_maf, max_sites=-1, flags=0, group_rows=0, chunk_bytes=0, pair_blocks=0):
    n = int(np.asarray(site_mask).shape[0])
    res = analyze_model.sites_scan(freq_text, depth_text, site_mask, sample_col, mean_depth, site_depth, site_ratio, allele_support,
                                   site_prev, site_maf, max_sites=max_sites, flags=(flags & abi.SITES_MASK_ONLY) | abi.SITES_SEQ,
                                   minor=np.full(n, MINOR, np.uint8), major=np.full(n, MAJOR, np.uint8), dump_keep=True)
    seq = res['seq']
    assert seq.shape[1] == int(res['keep'].sum())
    called, minor = seq != ord('-'), seq == MINOR
    S = seq.shape[0]
    both, diff = np.zeros((S, S), np.int64), np.zeros((S, S), np.int64)
    for i in range(S):
        for j in range(i, S):
            shared = called[i] & called[j]
            both[i, j] = int(shared.sum())
            diff[i, j] = int((shared & (minor[i] ^ minor[j])).sum())
    return dict(both=both, diff=diff, n_sites=res['n_sites'], n_kept=res['n_kept'], side_freq=res['side_freq'], side_depth=res['side_depth'])


def distances(both, diff):
    """diff / both above the diagonal, mirrored; the diagonal is 0."""
    n = both.shape[0]
    d = np.zeros((n, n), np.float64)
    for i in range(n):
        for j in range(i + 1, n):
            d[i, j] = d[j, i] = float(diff[i, j]) / float(both[i, j])
    return d


def nj_tree(dist):
    """Neighbour joining, the contract's arithmetic.  Every numpy expression below is elementwise fp64, one rounding each.  A
    row sum runs over the active slots in order with the row's own slot as +0.0: a sum that starts from +0.0 is never -0.0, so
    adding +0.0 leaves every bit as it is, and add.accumulate adds from left to right."""
    D = np.array(dist, np.float64)
    n = D.shape[0]
    assert D.shape == (n, n) and n >= 3
    active = list(range(n))
    join, length = [], []
    r = n
    while r > 3:
        act = np.array(active)
        sub = D[np.ix_(act, act)]
        terms = sub.copy()
        terms[np.arange(r), np.arange(r)] = 0.0
        R = np.add.accumulate(np.concatenate([np.zeros((r, 1)), terms], axis=1), axis=1)[:, -1]
        q = ((float(r - 2) * sub) - R[:, None]) - R[None, :]
        q[np.tril_indices(r)] = np.inf
        at = int(np.argmin(q))                  # the first of the least values, row by row: the smaller a, then the smaller b
        ia, ib = divmod(at, r)
        assert ia < ib
        a, b = active[ia], active[ib]
        dab = float(D[a, b])
        la = 0.5 * dab + (float(R[ia]) - float(R[ib])) / (2.0 * float(r - 2))
        lb = dab - la
        ks = np.array([k for k in active if k != a and k != b])
        new = 0.5 * ((D[a, ks] + D[b, ks]) - dab)
        D[a, ks] = new
        D[ks, a] = new
        active.remove(b)
        join.append((a, b))
        length.append((la, lb))
        r -= 1
    a, b, c = active
    ab, ac, bc = float(D[a, b]), float(D[a, c]), float(D[b, c])
    last_len = [0.5 * ((ab + ac) - bc), 0.5 * ((ab + bc) - ac), 0.5 * ((ac + bc) - ab)]
    return dict(join=np.array(join, np.int32).reshape(-1, 2), len=np.array(length, np.float64).reshape(-1, 2),
                last=np.array(active, np.int32), last_len=np.array(last_len, np.float64))


def newick(names, tree):
    node = list(names)
    for (a, b), (la, lb) in zip(tree['join'].tolist(), tree['len'].tolist()):
        node[a] = '(%s:%r,%s:%r)' % (node[a], la, node[b], lb)
    return '(%s);\n' % ','.join('%s:%r' % (node[k], x) for k, x in zip(tree['last'].tolist(), tree['last_len'].tolist()))


def pairs_table(names, both, diff, d):
    rows = ['\t'.join(['sample1', 'sample2', 'sites', 'mismatches', 'distance'])]
    for i in range(len(names)):
        for j in range(i + 1, len(names)):
            rows.append('%s\t%s\t%d\t%d\t%r' % (names[i], names[j], both[i, j], diff[i, j], float(d[i, j])))
    return '\n'.join(rows) + '\n'


def expected_files(argv):
    """-> (Newick text, pair table) of `snp_trees.py argv`, by this model alone; the argument parser, the sample selection and
    the site mask are the command's own."""
    args = cli.trees_arguments(argv)
    tables = sites.open_tables(args['indir'])
    samples = sites.fetch_samples(tables, args['sample_depth'], args['fract_cov'], args['max_samples'], args['keep_samples'],
                                  args['exclude_samples'])
    order = list(samples.values())
    mask, flags = trees.site_mask(args, tables)
    res = sites_consensus_pairs(tables.freq_text, tables.depth_text, np.ascontiguousarray(mask, np.uint8), [s.index for s in order],
                                [s.mean_depth for s in order], int(args['site_depth']), float(args['site_ratio']), float(args['allele_support']),
                                float(args['site_prev']), float(args['site_maf']),
                                max_sites=-1 if args['max_sites'] == float('inf') else int(args['max_sites']), flags=flags)
    d = distances(res['both'], res['diff'])
    names = list(samples)
    return newick(names, nj_tree(d)), pairs_table(names, res['both'], res['diff'], d)


class ModelContext:
    """Stands in for abi.Context in trees.run_pipeline.  sample_limit: what the device's free memory would hold."""

    def __init__(self, sample_limit=1 << 20):
        self.sample_limit = sample_limit

    def sites_consensus_pairs(self, freq_text, depth_text, site_mask, sample_col, *a, **kw):
        if len(sample_col) > self.sample_limit:
            e = abi.MidasSnpsError(abi.ERR_OUT_OF_MEMORY, "%d samples: the pair matrices of at most %d samples fit the free device memory"
                                   % (len(sample_col), self.sample_limit))
            e.bad, e.limit = None, self.sample_limit
            raise e
        try:
            return sites_consensus_pairs(freq_text, depth_text, site_mask, sample_col, *a, **kw)
        except analyze_model.BadCell as e:
            e.limit = None
            raise

    def nj_tree(self, dist):
        return nj_tree(dist)

    def close(self):
        pass


# ---- test inputs ---------------------------------------------------------------------------------------------------------------
def random_tree(n, rng):
    """A random unrooted binary tree on the leaves 0..n-1 with branch lengths k / 1024, k in 1..64 -> (the path-length matrix,
    {split: length}); a split is the leaf set on the side of a branch that leaf 0 is not on."""
    edges = {(0, n): 0, (1, n): 0, (2, n): 0}
    inner = n + 1
    for leaf in range(3, n):
        u, v = sorted(edges)[int(rng.integers(len(edges)))]
        del edges[(u, v)]
        edges.update({(u, inner): 0, (inner, v): 0, (leaf, inner): 0})
        inner += 1
    edges = {e: int(rng.integers(1, 65)) / 1024.0 for e in sorted(edges)}
    near = {}
    for (u, v), x in edges.items():
        near.setdefault(u, []).append((v, x))
        near.setdefault(v, []).append((u, x))

    def walk(start, banned):
        """{node: path length from start}, never stepping onto `banned`."""
        seen, stack = {start: 0.0}, [start]
        while stack:
            u = stack.pop()
            for v, x in near[u]:
                if v not in seen and v != banned:
                    seen[v] = seen[u] + x
                    stack.append(v)
        return seen

    dist = np.zeros((n, n))
    for i in range(n):
        far = walk(i, None)
        dist[i] = [far[j] for j in range(n)]
    splits = {}
    for (u, v), x in edges.items():
        side = frozenset(k for k in walk(v, u) if k < n)
        splits[side if 0 not in side else frozenset(range(n)) - side] = x
    assert len(splits) == 2 * n - 3
    return dist, splits


def tree_splits(n, tree):
    """{split: length} of a neighbour-joining result, in random_tree's terms."""
    leaves = [frozenset([k]) for k in range(n)]
    splits = {}

    def add(side, x):
        side = side if 0 not in side else frozenset(range(n)) - side
        assert side not in splits
        splits[side] = x

    for (a, b), (la, lb) in zip(tree['join'].tolist(), tree['len'].tolist()):
        add(leaves[a], la)
        add(leaves[b], lb)
        leaves[a] = leaves[a] | leaves[b]
    for k, x in zip(tree['last'].tolist(), tree['last_len'].tolist()):
        add(leaves[k], x)
    return splits


def star_matrix(n, c=0.5):
    return np.full((n, n), c) - np.eye(n) * c


def star_joins(n):
    """What the tie rule makes of a star: every Q value of every step is the same number, so slot 0 takes the least slot left."""
    return [(0, k) for k in range(1, n - 2)]


def ratio_matrix(n, rng, most=6):
    """diff / both of small random integers: many equal distances, hence equal Q values, and some negative lengths."""
    both = rng.integers(1, most + 1, (n, n))
    diff = rng.integers(0, most + 1, (n, n)) % (both + 1)
    d = np.triu(diff.astype(np.float64) / both.astype(np.float64), 1)
    return d + d.T


def zero_depth_column(indir, k):
    """Every depth of matrix column k becomes 0."""
    path = os.path.join(indir, 'snps_depth.txt')
    with open(path) as f:
        lines = f.read().split('\n')
    for r in range(1, len(lines)):
        if lines[r]:
            cells = lines[r].split('\t')
            cells[1 + k] = '0'
            lines[r] = '\t'.join(cells)
    with open(path, 'w') as f:
        f.write('\n'.join(lines))
