"""The sequential model of gene_assoc.py: the contract restated without the device and without
midas_amd.analyze.genes_assoc.  The cells come from compare_genes_model.read_cells; a row's presence, midranks and tie term are
formed from the counting definitions; the statistic of a relabelling is the plain sum over the samples it marks (no digits, no
tiles); the p-values and the Benjamini-Hochberg step are written out again here in plain Python.  ModelContext stands in for
abi.Context in the host tests; the GPU tests compare every output array with stats()."""
import math

import numpy as np

from midas_amd import abi
from tests import compare_genes_model as CG


def bits_of(words, n):
    """uint64 words -> [n] 0 / 1"""
    return [(int(words[s >> 6]) >> (s & 63)) & 1 for s in range(n)]


def planes_for(used, n1, P, seed, n_samples):
    """The relabellings as the contract draws them -> uint64 [P, W]."""
    W = (n_samples + 63) // 64
    rng = np.random.default_rng(seed)
    planes = [[0] * W for _ in range(P)]
    for b in range(P):
        for k in rng.permutation(len(used))[:n1].tolist():
            c = used[k]
            planes[b][c >> 6] |= 1 << (c & 63)
    return np.array(planes, np.uint64).reshape(P, W)


def midranks(v):
    """-> (doubled midranks, tie term) of the values v by the counting definition."""
    v = np.asarray(v, np.float64)
    lt = (v[None, :] < v[:, None]).sum(axis=1)
    eq = (v[None, :] == v[:, None]).sum(axis=1)
    return (2 * lt + eq + 1).astype(np.int64), int((eq.astype(np.int64) ** 2 - 1).sum())


def stats(cells, used, case, planes, cutoff=0.35, dtype='presabs', min_present=1, min_absent=0):
    """cells f64 [S, rows]; used, case: column lists; planes uint64 [P, W] -> the arrays Context.genes_assoc returns."""
    S, G = cells.shape
    used = list(used)
    N, n1 = len(used), len(case)
    is_case = np.array([1 if c in set(case) else 0 for c in used], np.int64)
    planes = np.asarray(planes, np.uint64).reshape(-1, (S + 63) // 64)
    P = planes.shape[0]
    L = np.array([[(int(planes[b, c >> 6]) >> (c & 63)) & 1 for c in used] for b in range(P)], np.int64).reshape(P, N)
    rows, count, ccase, w, ties, exceed, products = [], [], [], [], [], [], []
    for r in range(G):
        v = [float(cells[c, r]) for c in used]
        present = np.array([1 if x > cutoff else 0 for x in v], np.int64)
        c = int(present.sum())
        if not (c >= min_present and N - c >= min_absent):
            continue
        a = int((present * is_case).sum())
        if dtype == 'presabs':
            rk, T = present, 0
        else:
            rk, T = midranks(v)
        w0 = int((rk * is_case).sum())
        s = L @ rk                                        # [P]: a(M_b) or w(M_b)
        if dtype == 'presabs':
            x0, x = N * w0 - n1 * c, N * s - n1 * c
        else:
            x0, x = w0 - n1 * (N + 1), s - n1 * (N + 1)
        rows.append(r), count.append(c), ccase.append(a), w.append(w0), ties.append(T)
        exceed.append(int((np.abs(x) >= abs(x0)).sum()))
        products.append(s)
    K = len(rows)
    arr = lambda v, dt: np.array(v, dt).reshape(-1)
    return dict(n_rows=G, n_samples=S, n_used=N, n_case=n1, n_perms=P, dtype=dtype, n_kept=K, row_of_slot=arr(rows, np.int32),
                count=arr(count, np.int32), count_case=arr(ccase, np.int32), w=arr(w, np.int64), ties=arr(ties, np.int64),
                exceed=arr(exceed, np.uint32), products=np.array(products, np.int32).reshape(K, P))


# ---- the p-values, restated ----------------------------------------------------------------------------------------------------
def fisher(a, c, n1, n2):
    N = n1 + n2
    lf = lambda k: math.lgamma(k + 1)
    logp = lambda x: (lf(n1) - lf(x) - lf(n1 - x)) + (lf(n2) - lf(c - x) - lf(n2 - c + x)) - (lf(N) - lf(c) - lf(N - c))
    bound = math.exp(logp(a)) * (1 + 1e-7)
    total = 0.0
    x = max(0, c - n2)
    while x <= min(n1, c):
        if math.exp(logp(x)) <= bound:
            total += math.exp(logp(x))
        x += 1
    return min(1.0, total)


def ranksum(w, T, n1, n2):
    """-> (U1, p)"""
    N = n1 + n2
    U1 = w / 2.0 - n1 * (n1 + 1) / 2.0
    mu = n1 * n2 / 2.0
    var = n1 * n2 / 12.0 * ((N + 1) - T / (N * (N - 1.0)))
    if var <= 0:
        return U1, 1.0
    return U1, math.erfc(max(0.0, abs(U1 - mu) - 0.5) / math.sqrt(var) / math.sqrt(2.0))


def bh(p):
    m = len(p)
    order = sorted(range(m), key=lambda k: p[k])          # (sorted() is stable)
    q = [0.0] * m
    best = None
    for j in range(m, 0, -1):
        v = (p[order[j - 1]] * float(m)) / float(j)
        best = v if best is None or v < best else best
        q[order[j - 1]] = min(1.0, best)
    return q


def columns(res):
    n1, N, P = res['n_case'], res['n_used'], res['n_perms']
    n2 = N - n1
    effect, p = [], []
    for k in range(res['n_kept']):
        c, w, T = int(res['count'][k]), int(res['w'][k]), int(res['ties'][k])
        if res['dtype'] == 'presabs':
            effect.append(w / n1 - (c - w) / n2)
            p.append(fisher(w, c, n1, n2))
        else:
            U1, pv = ranksum(w, T, n1, n2)
            effect.append(U1 / (n1 * n2))
            p.append(pv)
    out = dict(effect=effect, p_value=p, q_value=bh(p))
    if P > 0:
        out['p_perm'] = [(int(e) + 1) / (P + 1) for e in res['exceed']]
        out['q_perm'] = bh(out['p_perm'])
    return out


def table_text(gene_ids, res):
    t = columns(res)
    names = ['gene_id', 'count_case', 'count_control', 'effect', 'p_value', 'q_value'] + (['exceed', 'p_perm', 'q_perm'] if res['n_perms'] else [])
    rows = ['\t'.join(names)]
    for k in range(res['n_kept']):
        a, c = int(res['count_case'][k]), int(res['count'][k])
        f = [gene_ids[res['row_of_slot'][k]], a, c - a, t['effect'][k], t['p_value'][k], t['q_value'][k]]
        if res['n_perms']:
            f += [int(res['exceed'][k]), t['p_perm'][k], t['q_perm'][k]]
        rows.append('\t'.join(str(v) for v in f))
    return '\n'.join(rows) + '\n'


def read_groups(groups_text, sample_ids, case_label=None):
    """A well-formed --groups text -> (used columns, case columns)."""
    label = {}
    for line in groups_text.split('\n'):
        if not line.strip() or line.startswith('#') or line.split('\t')[0] == 'sample_id':
            continue
        id, lab = line.rstrip('\r').split('\t')[:2]
        label[id] = lab
    used = [k for k, id in enumerate(sample_ids) if id in label]
    labels = sorted({label[sample_ids[k]] for k in used}, key=lambda l: l.encode())
    assert len(labels) == 2
    case_label = case_label if case_label is not None else labels[1]
    return used, [k for k in used if label[sample_ids[k]] == case_label]


def split_matrix(matrix_text, options):
    """The text of genes_copynum.txt -> (sample ids in use, gene ids of the rows read, cells [S, rows])."""
    header, _, body = matrix_text.partition('\n')
    ids = header.rstrip('\r').split('\t')[1:]
    n_rows = body.count('\n') + (1 if body and not body.endswith('\n') else 0)
    if options.get('max_genes') is not None:
        n_rows = min(n_rows, options['max_genes'])
    S = options.get('max_samples') or len(ids)
    cells, _ = CG.read_cells(body, n_rows, S, len(ids))
    gene_ids = [line.rstrip('\r').split('\t')[0] for line in body.split('\n')[:n_rows]]
    return ids[:S], gene_ids, cells


def model_tables(matrix_text, groups_text, options):
    """The whole command over the texts of genes_copynum.txt and the --groups file -> (the table, stats()'s result)."""
    ids, gene_ids, cells = split_matrix(matrix_text, options)
    used, case = read_groups(groups_text, ids, options.get('case'))
    planes = planes_for(used, len(case), options.get('permutations', 0), options.get('seed', 0), len(ids))
    res = stats(cells, used, case, planes, options.get('cutoff', 0.35), options.get('dtype', 'presabs'), options.get('min_present', 1),
                options.get('min_absent', 0))
    return table_text(gene_ids, res), res


class ModelContext:
    """A CPU double of abi.Context for midas_amd.analyze.genes_assoc: the same call, the same result keys, the same errors."""

    def genes_assoc(self, text, n_rows, n_samples, n_columns, use, case, planes, cutoff=0.35, dtype='presabs', min_present=1,
                    min_absent=0, group_rows=0, chunk_bytes=0, form=1, products=False):
        try:
            cells, _ = CG.read_cells(text, n_rows, n_samples, n_columns)
        except CG.BadMatrix as b:
            e = abi.MidasSnpsError(abi.ERR_BAD_LAYOUT, str(b))
            e.bad = b.bad
            raise e
        u, c = bits_of(use, n_samples), bits_of(case, n_samples)
        used = [s for s in range(n_samples) if u[s]]
        if len(used) > 8191:
            e = abi.MidasSnpsError(abi.ERR_UNSUPPORTED, "%d used samples" % len(used))
            e.bad = None
            raise e
        res = stats(cells, used, [s for s in used if c[s]], planes, cutoff, dtype, min_present, min_absent)
        if not products:
            del res['products']
        res.update(groups=1, form=form)
        return res

    def close(self):
        pass


def run(indir, groups, options, out, make_context):
    """gene_assoc.py in process -> (what it printed, the table)."""
    import contextlib
    import io
    from midas_amd.analyze import cli, genes_assoc
    args = cli.gene_assoc_arguments([indir, '--groups', groups, '--out', out] + list(options))
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        genes_assoc.assoc(args, make_context=make_context)
    with open(out) as f:
        return buf.getvalue(), f.read()
