"""The sequential model of gene_curves.py: the contract as plain numpy, no device and no genes_curves.py.
The cells come from compare_genes_model.read_cells; for every order np.cumsum of the permuted presence columns gives
c(g, r, k), and pan, core and single are the counts of c >= 1, c >= need[k] and c == 1; need[] comes from a linear search; both
tables and the Heaps line are written as text.  device_call stands in for abi.genes_curves in the host tests; the GPU tests
compare every output array with curves()."""
import math

import numpy as np

from midas_amd import abi
from tests import compare_genes_model as CG
from tests.gene_linkage_model import matrix_text, split_matrix  # noqa: F401  (the host tests build their matrices with these)

STAT_COLUMNS = ['pan_mean', 'pan_min', 'pan_max', 'core_mean', 'core_min', 'core_max', 'single_mean', 'single_min', 'single_max', 'new_mean']


def need_linear(n_used, t):
    """need[k] = the smallest n in [1, k] with float(n) / float(k) >= t, by trying n = 1, 2, ...; need[0] = 0 (unused)."""
    need = [0]
    for k in range(1, n_used + 1):
        n = 1
        while not float(n) / float(k) >= t:
            n += 1
        need.append(n)
    return need


def orders_model(used, P, seed):
    used = sorted(int(c) for c in used)
    rng = np.random.default_rng(seed)
    return np.array([used] + [[used[j] for j in rng.permutation(len(used))] for _ in range(P)], np.int32).reshape(1 + P, len(used))


def curves(cells, cutoff, orders, need):
    """cells f64 [S, rows] -> dict(pan, core, single: int64 [R, N])."""
    present = (cells > cutoff).astype(np.int64)              # [S, rows]
    orders = np.asarray(orders)
    R, N = orders.shape
    nd = np.asarray(need, np.int64)[1:N + 1][:, None]
    out = {k: np.zeros((R, N), np.int64) for k in ('pan', 'core', 'single')}
    for r in range(R):
        c = np.cumsum(present[orders[r]], axis=0)            # [N, rows]: the count after k = 1 .. N samples
        out['pan'][r] = (c >= 1).sum(axis=1)
        out['core'][r] = (c >= nd).sum(axis=1)
        out['single'][r] = (c == 1).sum(axis=1)
    return out


def stat_columns(res):
    """-> {column: list over k} of the ten statistic columns, or {} without a random order."""
    P = res['pan'].shape[0] - 1
    if P < 1:
        return {}
    out = {}
    for name in ('pan', 'core', 'single'):
        rows = [[int(v) for v in row] for row in res[name][1:]]
        total = [sum(col) for col in zip(*rows)]
        out[name + '_mean'] = [float(t) / float(P) for t in total]
        out[name + '_min'] = [min(col) for col in zip(*rows)]
        out[name + '_max'] = [max(col) for col in zip(*rows)]
        if name == 'pan':
            out['new_mean'] = [float(t - (total[k - 1] if k else 0)) / float(P) for k, t in enumerate(total)]
    return out


def curves_text(res):
    P = res['pan'].shape[0] - 1
    st = stat_columns(res)
    rows = ['\t'.join(['samples', 'pan', 'core', 'single', 'new'] + (STAT_COLUMNS if P else []))]
    pan = [int(v) for v in res['pan'][0]]
    for k in range(len(pan)):
        row = [k + 1, pan[k], int(res['core'][0][k]), int(res['single'][0][k]), pan[k] - (pan[k - 1] if k else 0)]
        row += [st[c][k] for c in STAT_COLUMNS] if P else []
        rows.append('\t'.join(str(v) for v in row))
    return '\n'.join(rows) + '\n'


def orders_text(sample_ids, res, orders):
    rows = ['\t'.join(['order', 'samples', 'sample_id', 'pan', 'core', 'single'])]
    R, N = res['pan'].shape
    for r in range(R):
        for k in range(N):
            rows.append('\t'.join(str(v) for v in [r, k + 1, sample_ids[int(orders[r][k])], int(res['pan'][r][k]), int(res['core'][r][k]),
                                                   int(res['single'][r][k])]))
    return '\n'.join(rows) + '\n'


def heaps_line(new):
    """new[k - 1] for k = 1 .. N -> the line gene_curves.py prints."""
    pts = [(math.log(k), math.log(float(v))) for k, v in enumerate(new, 1) if k >= 2 and v > 0]
    n = len(pts)
    if n < 2:
        return "Heaps' law: not fitted"
    mx = math.fsum(x for x, _ in pts) / n
    my = math.fsum(y for _, y in pts) / n
    slope = math.fsum((x - mx) * (y - my) for x, y in pts) / math.fsum((x - mx) ** 2 for x, _ in pts)
    alpha, K = -slope, math.exp(my - slope * mx)
    return "Heaps' law: alpha %s, K %s: %s" % (repr(alpha), repr(K), 'open' if alpha <= 1 else 'closed')


def new_of(res):
    """The values Heaps' law is fitted to: new_mean with random orders, order 0's new without."""
    st = stat_columns(res)
    if st:
        return st['new_mean']
    pan = [int(v) for v in res['pan'][0]]
    return [pan[k] - (pan[k - 1] if k else 0) for k in range(len(pan))]


def read_samples_model(lines, sample_ids):
    """The ids of a --samples file's lines -> the columns they name, ascending (no error handling: the tests' files are good)."""
    ids = [l.split('\t')[0] for l in lines if l.strip() and not l.startswith('#')]
    return sorted({sample_ids.index(i) for i in ids})


def model_tables(matrix_text_, options, sample_lines=None):
    """The whole command over the text of genes_copynum.txt -> (curve table, orders table, curves()'s result with orders, need,
    n_rows, the stdout lines)."""
    header = matrix_text_.partition('\n')[0]
    ids = header.split('\t')[1:]
    _, cells = split_matrix(matrix_text_, options)
    S = cells.shape[0]
    used = read_samples_model(sample_lines, ids[:S]) if sample_lines is not None else list(range(S))
    P, seed = options.get('permutations', 100), options.get('seed', 0)
    orders = orders_model(used, P, seed)
    need = need_linear(len(used), options.get('core_frac', 1.0))
    res = curves(cells, options.get('cutoff', 0.35), orders, need)
    N = len(used)
    lines = ["Rows read: %d" % cells.shape[1], "Samples in use: %d of %d" % (N, S), "Orders: the listed one and %d random (seed %d)" % (P, seed),
             "All %d samples: pan %d, core %d (present in >= %d), single %d" % (N, res['pan'][0][N - 1], res['core'][0][N - 1], need[N],
                                                                                res['single'][0][N - 1]),
             heaps_line(new_of(res))]
    res.update(orders=orders, need=need, n_rows=cells.shape[1], lines=lines)
    return curves_text(res), orders_text(ids, res, orders), res


def device_call(ctx, text, n_rows, n_samples, n_columns, orders, need, cutoff=0.35, form=1, group_rows=0, chunk_bytes=0, out=None):
    """A CPU double of abi.genes_curves: the same call, the same result keys, the same errors."""
    try:
        cells, _ = CG.read_cells(text, n_rows, n_samples, n_columns)
    except CG.BadMatrix as b:
        e = abi.MidasSnpsError(abi.ERR_BAD_LAYOUT, str(b))
        e.bad = b.bad
        raise e
    orders = np.asarray(orders, np.int32)
    res = curves(cells, cutoff, orders, [int(x) for x in need])
    res.update(n_rows=cells.shape[1], n_samples=n_samples, n_used=orders.shape[1], n_orders=orders.shape[0], groups=1, form=form, planes=0, words=0)
    return res


class ModelContext:
    def close(self):
        pass


def run(indir, options, out, orders_path=None):
    """gene_curves.py in process over the model's device_call -> (what it printed, the curve table, the orders table or None)."""
    import contextlib
    import io
    from midas_amd.analyze import cli, genes_curves
    argv = [indir, '--out', out] + (['--orders', orders_path] if orders_path else []) + list(options)
    args = cli.gene_curves_arguments(argv)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        genes_curves.curves(args, make_context=ModelContext, device_call=device_call)
    with open(out) as f:
        table = f.read()
    if not orders_path:
        return buf.getvalue(), table, None
    with open(orders_path) as f:
        return buf.getvalue(), table, f.read()
