"""MI355X-native gene_curves.py: the host side.

Not a command of the reference.  Only genes_copynum.txt is read; it is mapped and handed to the device as text, under the
header checks, --max_genes / --max_samples rules and cell errors of compare_genes.py (genes_compare.select).  One device call
(midas_genes_curves) calls presence and counts, for the listed order of the samples and for --permutations random orders, the
genes found in at least one, in at least need[k] and in exactly one of the first k samples, k = 1 .. N (DESIGN.md section 23
has the contract).  Every number that comes back is an integer.

The host makes the orders (orders_table: an input of the device call, so that its result is a function of its arguments
alone) and need[] (need_table: --core_frac by bisection over the fp64 expression the contract names, so the device divides
nothing), forms the means over the random orders from integer sums, and fits Heaps' law to the new genes a sample.  Both
tables are written natively.
"""
import math
import sys

import numpy as np

from midas_amd import abi
from midas_amd.analyze import genes_compare
from midas_amd.analyze import sites as S

_exit = genes_compare._exit

MAX_USED = 8191
MAX_PERMUTATIONS = 100000
STAT_COLUMNS = ('pan_mean', 'pan_min', 'pan_max', 'core_mean', 'core_min', 'core_max', 'single_mean', 'single_min', 'single_max', 'new_mean')


def need_table(n_used, core_frac):
    """-> int32 [n_used + 1]: need[k] = the smallest n in [1, k] with float(n) / float(k) >= core_frac (0 < core_frac <= 1, so
    n = k always qualifies; the quotient does not fall as n grows).  need[0] = 0 is never used.  n >= 1: a gene found in none
    of the k samples is never core."""
    t = float(core_frac)
    need = np.zeros(int(n_used) + 1, np.int32)
    for k in range(1, int(n_used) + 1):
        lo, hi = 1, k                       # the answer lies in [lo, hi]; hi qualifies
        while lo < hi:
            mid = (lo + hi) // 2
            if float(mid) / float(k) >= t:
                hi = mid
            else:
                lo = mid + 1
        need[k] = hi
    return need


def read_samples(path, sample_ids):
    """The --samples file against the sample ids of the columns in use -> the columns it names, ascending.  One id a line, in
    the first tab field; blank lines and # lines are skipped, a repeated id counts once.  Every broken rule ends with the Error
    exit that names the file and the line."""
    column = {id: k for k, id in enumerate(sample_ids)}
    used = set()
    try:
        f = open(path, encoding='utf-8', errors='surrogateescape', newline='')
    except OSError:
        _exit("%s: cannot be read" % path)
    with f:
        for n, line in enumerate(f, 1):
            line = line.rstrip('\n').rstrip('\r')
            if not line.strip() or line.startswith('#'):
                continue
            id = line.split('\t')[0]
            if id not in column:
                _exit("%s, line %d: the sample %s is not among the %d sample columns in use" % (path, n, id, len(sample_ids)))
            used.add(column[id])
    if not used:
        _exit("%s: names no sample" % path)
    return sorted(used)


def orders_table(used_columns, P, seed):
    """-> int32 [1 + P, N]: row 0 the used columns ascending, row r >= 1 used[rng.permutation(N)], rng =
    np.random.default_rng(seed) drawn from row 1 on."""
    used = np.sort(np.asarray(used_columns, np.int32))
    orders = np.empty((1 + int(P), used.shape[0]), np.int32)
    orders[0] = used
    rng = np.random.default_rng(seed)
    for r in range(1, 1 + int(P)):
        orders[r] = used[rng.permutation(used.shape[0])]
    return orders


def table_columns(res):
    """What genes_curves returned -> the ten statistic columns over the random orders (rows 1 .. P), or {} when P = 0: the means
    are float(integer sum) / float(P), new_mean the difference of pan's sums at k and k - 1 over float(P); min and max int64."""
    P = int(res['pan'].shape[0]) - 1
    if P < 1:
        return {}
    out = {}
    sums = {}
    for name in ('pan', 'core', 'single'):
        a = np.asarray(res[name], np.int64)[1:]
        sums[name] = [int(v) for v in a.sum(axis=0)]
        out[name + '_mean'] = np.array([float(v) / float(P) for v in sums[name]], np.float64).reshape(-1)
        out[name + '_min'], out[name + '_max'] = a.min(axis=0), a.max(axis=0)
    sp = sums['pan']
    out['new_mean'] = np.array([float(sp[k] - (sp[k - 1] if k else 0)) / float(P) for k in range(len(sp))], np.float64).reshape(-1)
    return out


def heaps_fit(new):
    """new[k - 1] = the genes sample k adds, k = 1 .. N -> (alpha, K, open) of new ~ K k^-alpha by least squares over the points
    k >= 2 with new > 0 in log-log space, or None with fewer than two points."""
    pts = [(math.log(k), math.log(float(v))) for k, v in enumerate(new, 1) if k >= 2 and v > 0]
    n = len(pts)
    if n < 2:
        return None
    mx, my = math.fsum(x for x, _ in pts) / n, math.fsum(y for _, y in pts) / n
    slope = math.fsum((x - mx) * (y - my) for x, y in pts) / math.fsum((x - mx) ** 2 for x, _ in pts)
    alpha, K = -slope, math.exp(my - slope * mx)
    return alpha, K, alpha <= 1


def heaps_line(new):
    fit = heaps_fit(new)
    if fit is None:
        return "Heaps' law: not fitted"
    return "Heaps' law: alpha %s, K %s: %s" % (repr(fit[0]), repr(fit[1]), 'open' if fit[2] else 'closed')


def curves(args, make_context=S.device_context, device_call=abi.genes_curves):
    """The command.  device_call: tests substitute a model of abi.genes_curves."""
    print("Reading gene copy-number matrix\n")
    matrix = genes_compare.open_matrix(args['copynum'])
    n_rows, n_samples = genes_compare.select(matrix, args['max_genes'], args['max_samples'])
    used = read_samples(args['samples'], matrix.sample_ids[:n_samples]) if args.get('samples') else list(range(n_samples))
    if len(used) > MAX_USED:
        _exit("%d samples are in use, more than %d: use --max_samples or --samples" % (len(used), MAX_USED))
    P, seed = int(args['permutations']), int(args['seed'])
    orders = orders_table(used, P, seed)
    need = need_table(len(used), args['core_frac'])
    ctx = make_context()
    try:
        res = device_call(ctx, matrix.text, n_rows, n_samples, matrix.n_columns, orders, need, cutoff=float(args['cutoff']),
                          form=int(args.get('form', 1)), group_rows=int(args.get('group_rows', 0) or 0),
                          chunk_bytes=int(args.get('chunk_bytes', 0) or 0))
    except abi.MidasSnpsError as e:
        genes_compare.exit_bad_row(matrix, e)
    finally:
        ctx.close()
    table = table_columns(res)
    N = len(used)
    pan0 = [int(v) for v in res['pan'][0]]
    new = table['new_mean'].tolist() if P else [pan0[k] - (pan0[k - 1] if k else 0) for k in range(N)]
    print("Rows read: %d" % res['n_rows'])
    print("Samples in use: %d of %d" % (N, n_samples))
    print("Orders: the listed one and %d random (seed %d)" % (P, seed))
    print("All %d samples: pan %d, core %d (present in >= %d), single %d"
          % (N, pan0[N - 1], int(res['core'][0][N - 1]), int(need[N]), int(res['single'][0][N - 1])))
    print(heaps_line(new) + "\n")
    sys.stdout.flush()
    try:
        matrix.write_curves(args['out'], res, table)
        if args.get('orders'):
            matrix.write_curve_orders(args['orders'], res, orders)
    except abi.MidasSnpsError as e:
        _exit(e.message)
    res.update(table=table, orders=orders, need=need)
    return res
