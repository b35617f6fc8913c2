"""The sequential model of gene_linkage.py: the contract as plain Python, no device.  The cells come from
compare_genes_model.read_cells; a gene's presence is a Python integer used as a bit mask; need[] comes from a linear search;
the pairs from two nested loops; the components from a plain union-find reduced to the smallest slot; both tables are written
as text.  ModelContext stands in for abi.Context in the host tests; the GPU tests compare every output array with link()."""
import numpy as np

from midas_amd import abi
from tests import compare_genes_model as CG


def need_linear(n_samples, t):
    """need[u] = the smallest n in [0, u] with float(n) / float(u) >= t, by trying n = 0, 1, 2, ...; need[0] = 0 (unused)."""
    need = [0]
    for u in range(1, n_samples + 1):
        n = 0
        while not float(n) / float(u) >= t:
            n += 1
        need.append(n)
    return need


def masks(cells, cutoff):
    """cells f64 [S, rows] -> one int a row: bit s set when the gene is present in sample s."""
    S, G = cells.shape
    return [sum(1 << s for s in range(S) if cells[s, r] > cutoff) for r in range(G)]


def link(cells, cutoff, min_present, min_absent, need):
    """-> dict(count, row_of_slot, label, pair_a, pair_b, pair_both: int32 arrays; visited, linked)."""
    S, G = cells.shape
    m = masks(cells, cutoff)
    c = [bin(x).count('1') for x in m]
    rows = [r for r in range(G) if c[r] >= min_present and S - c[r] >= min_absent]
    K = len(rows)
    pa, pb, pc = [], [], []
    for a in range(K):
        for b in range(a + 1, K):
            both = bin(m[rows[a]] & m[rows[b]]).count('1')
            either = c[rows[a]] + c[rows[b]] - both
            if both >= need[either]:
                pa.append(a)
                pb.append(b)
                pc.append(both)
    parent = list(range(K))

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x
    for a, b in zip(pa, pb):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    label = [find(k) for k in range(K)]
    i32 = lambda v: np.array(v, np.int32).reshape(-1)
    return dict(n_rows=G, n_samples=S, n_kept=K, count=i32([c[r] for r in rows]), row_of_slot=i32(rows), label=i32(label), pair_a=i32(pa),
                pair_b=i32(pb), pair_both=i32(pc), visited=K * (K - 1) // 2, linked=len(pa))


def pairs_text(gene_ids, res):
    rows = ['\t'.join(['gene1', 'gene2', 'count1', 'count2', 'count_both', 'count_either', 'jaccard'])]
    for a, b, both in zip(res['pair_a'].tolist(), res['pair_b'].tolist(), res['pair_both'].tolist()):
        c1, c2 = int(res['count'][a]), int(res['count'][b])
        either = c1 + c2 - both
        rows.append('\t'.join(str(v) for v in [gene_ids[res['row_of_slot'][a]], gene_ids[res['row_of_slot'][b]], c1, c2, both, either,
                                               repr(float(both) / either)]))
    return '\n'.join(rows) + '\n'


def groups_text(gene_ids, res, min_group):
    """-> (the table, the number of groups)"""
    rows = ['\t'.join(['group_id', 'group_size', 'gene_id', 'count'])]
    label = res['label'].tolist()
    n = 0
    for r in range(len(label)):
        if label[r] != r:
            continue
        members = [k for k in range(len(label)) if label[k] == r]
        if len(members) < min_group:
            continue
        n += 1
        for k in members:
            rows.append('\t'.join(str(v) for v in [n, len(members), gene_ids[res['row_of_slot'][k]], int(res['count'][k])]))
    return '\n'.join(rows) + '\n', n


def split_matrix(matrix_text, options):
    """The text of genes_copynum.txt -> (gene ids of the rows read, cells [S, rows])."""
    header, _, body = matrix_text.partition('\n')
    ids = header.split('\t')[1:]
    n_rows = body.count('\n') + (1 if body and not body.endswith('\n') else 0)
    if options.get('max_genes') is not None:
        n_rows = min(n_rows, options['max_genes'])
    S = options.get('max_samples') or len(ids)
    cells, _ = CG.read_cells(body, n_rows, S, len(ids))
    gene_ids = [line.rstrip('\r').split('\t')[0] for line in body.split('\n')[:n_rows]]
    return gene_ids, cells


def model_tables(matrix_text, options):
    """The whole command over the text of genes_copynum.txt -> (pair table, group table, link()'s result)."""
    gene_ids, cells = split_matrix(matrix_text, options)
    need = need_linear(cells.shape[0], options.get('min_jaccard', 0.9))
    res = link(cells, options.get('cutoff', 0.35), options.get('min_present', 2), options.get('min_absent', 2), need)
    return pairs_text(gene_ids, res), groups_text(gene_ids, res, options.get('min_group', 2))[0], res


class ModelContext:
    """A CPU double of abi.Context for midas_amd.analyze.genes_linkage: the same call, the same result keys, the same errors."""

    def genes_linkage(self, text, n_rows, n_samples, n_columns, need, cutoff=0.35, min_present=2, min_absent=2, max_pairs=1 << 26,
                      group_rows=0, chunk_bytes=0, pair_form=0, pair_out=None):
        try:
            cells, _ = CG.read_cells(text, n_rows, n_samples, n_columns)
        except CG.BadMatrix as b:
            e = abi.MidasSnpsError(abi.ERR_BAD_LAYOUT, str(b))
            e.bad = b.bad
            raise e
        res = link(cells, cutoff, min_present, min_absent, [int(x) for x in need])
        if res['linked'] > max_pairs:
            e = abi.MidasSnpsError(abi.ERR_OUT_OF_MEMORY, "%d linked pairs of genes, but max_pairs is %d" % (res['linked'], max_pairs))
            e.bad, e.linked = None, res['linked']
            raise e
        res.update(label_rounds=0, groups=1)
        return res

    def close(self):
        pass


def matrix_text(gene_ids, sample_ids, present, hi='1.5', lo='0.0'):
    """A genes_copynum.txt whose cell (g, s) is `hi` where present[g][s] and `lo` elsewhere."""
    rows = ['\t'.join(['gene_id'] + list(sample_ids))]
    for g, id in enumerate(gene_ids):
        rows.append('\t'.join([id] + [hi if present[g][s] else lo for s in range(len(sample_ids))]))
    return '\n'.join(rows) + '\n'


def run(indir, options, out, groups, make_context):
    """gene_linkage.py in process -> (what it printed, the pair table, the group table or None)."""
    import contextlib
    import io
    from midas_amd.analyze import cli, genes_linkage
    argv = [indir, '--out', out] + (['--groups', groups] if groups else []) + list(options)
    args = cli.gene_linkage_arguments(argv)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        genes_linkage.link(args, make_context=make_context)
    with open(out) as f:
        pairs = f.read()
    if not groups:
        return buf.getvalue(), pairs, None
    with open(groups) as f:
        return buf.getvalue(), pairs, f.read()
