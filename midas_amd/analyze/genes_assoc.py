"""MI355X-native gene_assoc.py: the host side.

Not a command of the reference.  Only genes_copynum.txt is read; it is mapped and handed to the device as text, under the
header checks, --max_genes / --max_samples rules and cell errors of compare_genes.py (genes_compare.select).  --groups names
two groups of samples; one device call (midas_genes_assoc) calls presence, keeps the genes --min_present / --min_absent allow,
forms the counts or the doubled midranks and their sum over the cases, and counts the relabellings of the samples whose
statistic is at least as extreme (DESIGN.md section 22 has the contract).  Every number that comes back is an integer.

The host makes the relabellings (permutation_planes: an input of the device call, so that its result is a function of its
arguments alone) and turns the integers into p-values: Fisher's exact test or the rank-sum test with tie and continuity
correction, the permutation p-value, and Benjamini-Hochberg q-values, each operation in the order the contract writes it.  The
table is written natively.
"""
import math
import sys

import numpy as np

from midas_amd import abi
from midas_amd.analyze import genes_compare
from midas_amd.analyze import sites as S

_exit = genes_compare._exit

MAX_USED = 8191
MAX_PERMUTATIONS = 1000000


def words_of(columns, n_samples):
    """-> uint64 [ceil(n_samples / 64)] with the bits `columns` set."""
    w = np.zeros((int(n_samples) + 63) // 64, np.uint64)
    for c in columns:
        w[int(c) >> 6] |= np.uint64(1) << np.uint64(int(c) & 63)
    return w


def permutation_planes(used_columns, n1, P, seed, n_samples=None):
    """-> uint64 [P, W]: plane b has the bits used_columns[rng.permutation(N)[:n1]] set, rng = np.random.default_rng(seed) drawn
    from plane 0 on.  W = ceil(n_samples / 64) (n_samples: the sample columns in use; by default just past the last used one)."""
    used = np.asarray(used_columns, np.int64)
    N = used.shape[0]
    S_ = int(n_samples) if n_samples is not None else (int(used.max()) + 1 if N else 0)
    W = (S_ + 63) // 64
    planes = np.zeros((int(P), W), np.uint64)
    rng = np.random.default_rng(seed)
    one = np.uint64(1)
    for b in range(int(P)):
        cols = used[rng.permutation(N)[:n1]]
        np.bitwise_or.at(planes[b], cols >> 6, one << (cols & 63).astype(np.uint64))
    return planes


def read_groups(path, sample_ids, case_label=None):
    """The --groups file against the sample ids of the columns in use -> (used columns, case columns, control columns, case
    label, control label).  Every broken rule ends with the Error exit that names the file and the line."""
    column = {id: k for k, id in enumerate(sample_ids)}
    label_of, line_of = {}, {}
    try:
        f = open(path, encoding='utf-8', errors='surrogateescape', newline='')
    except OSError:
        _exit("%s: cannot be read" % path)
    with f:
        for n, line in enumerate(f, 1):
            line = line.rstrip('\n').rstrip('\r')
            if not line.strip() or line.startswith('#'):
                continue
            fields = line.split('\t')
            if len(fields) < 2 or not fields[0] or not fields[1]:
                _exit("%s, line %d: not sample_id<TAB>label" % (path, n))
            id, label = fields[0], fields[1]
            if id == 'sample_id':
                continue
            if id in label_of:
                if label_of[id] != label:
                    _exit("%s, line %d: the sample %s has the label %s here and %s on line %d" % (path, n, id, label, label_of[id], line_of[id]))
                continue
            label_of[id], line_of[id] = label, n
    labels = []
    for id in sorted((i for i in label_of if i in column), key=lambda i: line_of[i]):
        if label_of[id] not in labels:
            if len(labels) == 2:
                _exit("%s, line %d: a third label, %s, beside %s and %s" % (path, line_of[id], label_of[id], labels[0], labels[1]))
            labels.append(label_of[id])
    if case_label is None:
        if len(labels) < 2:
            _exit("%s: two groups are needed, but the samples of the matrix carry %s" %
                  (path, "the label %s only" % labels[0] if labels else "no label"))
        case_label = max(labels, key=lambda l: l.encode('utf-8', errors='surrogateescape'))
    elif case_label not in labels:
        _exit("%s: --case %s: no sample of the matrix has this label" % (path, case_label))
    elif len(labels) < 2:
        _exit("%s: two groups are needed, but the samples of the matrix carry the label %s only" % (path, labels[0]))
    control_label = labels[1] if labels[0] == case_label else labels[0]
    used = sorted(column[id] for id in label_of if id in column)
    case = [c for c in used if label_of[sample_ids[c]] == case_label]
    control = [c for c in used if label_of[sample_ids[c]] != case_label]
    if len(used) > MAX_USED:
        _exit("%s: %d samples of the matrix carry a label, more than %d" % (path, len(used), MAX_USED))
    return used, case, control, case_label, control_label


def log_factorials(n):
    return [math.lgamma(k + 1) for k in range(n + 1)]


def fisher_p(a, c, n1, n2, lf):
    """Fisher's exact test, two-sided: the sum of the table probabilities no greater than the observed one's."""
    N = n1 + n2

    def logp(x):
        return (lf[n1] - lf[x] - lf[n1 - x]) + (lf[n2] - lf[c - x] - lf[n2 - c + x]) - (lf[N] - lf[c] - lf[N - c])
    limit = math.exp(logp(a)) * (1 + 1e-7)
    total = 0.0
    for x in range(max(0, c - n2), min(n1, c) + 1):
        px = math.exp(logp(x))
        if px <= limit:
            total += px
    return min(1.0, total)


def ranksum_p(w, T, n1, n2):
    """-> (U1, p): the rank-sum test from the doubled rank sum w of the cases and the tie term T, normal approximation."""
    N = n1 + n2
    U1 = w / 2.0 - n1 * (n1 + 1) / 2.0
    mu = n1 * n2 / 2.0
    var = n1 * n2 / 12.0 * ((N + 1) - T / (N * (N - 1.0)))
    if var <= 0:
        return U1, 1.0
    return U1, math.erfc(max(0.0, abs(U1 - mu) - 0.5) / math.sqrt(var) / math.sqrt(2.0))


def benjamini_hochberg(p):
    """q_(j) = min(1, min over k >= j of p_(k) * m / k) over the stable ascending order of p."""
    p = np.asarray(p, np.float64)
    m = p.shape[0]
    if m == 0:
        return p.copy()
    order = np.argsort(p, kind='stable')
    v = (p[order] * float(m)) / np.arange(1, m + 1, dtype=np.float64)
    v = np.minimum(np.minimum.accumulate(v[::-1])[::-1], 1.0)
    q = np.empty(m, np.float64)
    q[order] = v
    return q


def table_columns(res):
    """What Context.genes_assoc returned -> dict(effect, p_value, q_value and, with permutations, p_perm, q_perm: f64 [K])."""
    n1, N, P = int(res['n_case']), int(res['n_used']), int(res['n_perms'])
    n2 = N - n1
    K = int(res['n_kept'])
    effect, p_value = np.zeros(K, np.float64), np.zeros(K, np.float64)
    count, w, ties = res['count'].tolist(), res['w'].tolist(), res['ties'].tolist()
    if res['dtype'] == 'presabs':
        lf = log_factorials(N)
        seen = {}
        for k in range(K):
            a, c = w[k], count[k]
            if (a, c) not in seen:
                seen[(a, c)] = fisher_p(a, c, n1, n2, lf)
            p_value[k] = seen[(a, c)]
            effect[k] = a / n1 - (c - a) / n2
    else:
        for k in range(K):
            U1, p_value[k] = ranksum_p(w[k], ties[k], n1, n2)
            effect[k] = U1 / (n1 * n2)
    out = dict(effect=effect, p_value=p_value, q_value=benjamini_hochberg(p_value))
    if P > 0:
        out['p_perm'] = np.array([(e + 1) / (P + 1) for e in res['exceed'].tolist()], np.float64).reshape(-1)
        out['q_perm'] = benjamini_hochberg(out['p_perm'])
    return out


def assoc(args, make_context=S.device_context):
    """The command.  make_context: tests substitute a CPU double of the device."""
    print("Reading gene copy-number matrix\n")
    matrix = genes_compare.open_matrix(args['copynum'])
    n_rows, n_samples = genes_compare.select(matrix, args['max_genes'], args['max_samples'])
    used, case, control, case_label, control_label = read_groups(args['groups'], matrix.sample_ids[:n_samples], args.get('case'))
    print("Samples used: %d (%d of the case group %s, %d of the control group %s)" % (len(used), len(case), case_label, len(control), control_label))
    print("Samples of the matrix without a label, left out: %d\n" % (n_samples - len(used)))
    P = int(args['permutations'])
    planes = permutation_planes(used, len(case), P, int(args['seed']), n_samples)
    ctx = make_context()
    try:
        res = ctx.genes_assoc(matrix.text, n_rows, n_samples, matrix.n_columns, words_of(used, n_samples), words_of(case, n_samples), planes,
                              cutoff=float(args['cutoff']), dtype=args['dtype'], min_present=int(args['min_present']),
                              min_absent=int(args['min_absent']), group_rows=int(args.get('group_rows', 0) or 0),
                              chunk_bytes=int(args.get('chunk_bytes', 0) or 0), form=int(args.get('form', 1)))
    except abi.MidasSnpsError as e:
        genes_compare.exit_bad_row(matrix, e)
    finally:
        ctx.close()
    print("Rows read: %d" % res['n_rows'])
    print("Genes kept (present in >= %d and absent from >= %d of %d samples): %d"
          % (args['min_present'], args['min_absent'], len(used), res['n_kept']))
    if P:
        print("Relabellings of the samples: %d (seed %d)" % (P, args['seed']))
    print("")
    sys.stdout.flush()
    table = table_columns(res)
    try:
        matrix.write_assoc(args['out'], res, table)
    except abi.MidasSnpsError as e:
        _exit(e.message)
    res['table'] = table
    return res
