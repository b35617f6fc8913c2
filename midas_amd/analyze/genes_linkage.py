"""MI355X-native gene_linkage.py: the host side.

Not a command of the reference.  Only genes_copynum.txt is read; it is mapped and handed to the device as text, under the
header checks, --max_genes / --max_samples rules and cell errors of compare_genes.py (genes_compare.select).  One device call
calls presence, keeps the genes --min_present / --min_absent allow, tests every pair of kept genes and labels the connected
components of the linked pairs; both tables are written natively (DESIGN.md section 21 has the contract).

The device divides nothing: need_table() turns --min_jaccard into the fewest shared samples that link a pair at every size of
the union, by bisection over the fp64 expression the contract names.
"""
import sys

import numpy as np

from midas_amd import abi
from midas_amd.analyze import genes_compare
from midas_amd.analyze import sites as S

_exit = genes_compare._exit


def need_table(n_samples, min_jaccard):
    """-> int32 [n_samples + 1]: need[u] = the smallest n in [0, u] with float(n) / float(u) >= min_jaccard (0 < min_jaccard <= 1,
    so n = u always qualifies; the quotient does not fall as n grows).  need[0] = 0 is never used."""
    t = float(min_jaccard)
    need = np.zeros(int(n_samples) + 1, np.int32)
    for u in range(1, int(n_samples) + 1):
        lo, hi = 0, u                       # the answer lies in [lo, hi]; hi qualifies
        while lo < hi:
            mid = (lo + hi) // 2
            if float(mid) / float(u) >= t:
                hi = mid
            else:
                lo = mid + 1
        need[u] = hi
    return need


def link(args, make_context=S.device_context):
    """The command.  make_context: tests substitute a CPU double of the device."""
    print("Reading gene copy-number matrix\n")
    matrix = genes_compare.open_matrix(args['copynum'])
    n_rows, n_samples = genes_compare.select(matrix, args['max_genes'], args['max_samples'])
    need = need_table(n_samples, args['min_jaccard'])
    ctx = make_context()
    try:
        res = ctx.genes_linkage(matrix.text, n_rows, n_samples, matrix.n_columns, need, cutoff=float(args['cutoff']),
                                min_present=int(args['min_present']), min_absent=int(args['min_absent']), max_pairs=int(args['max_pairs']),
                                group_rows=int(args.get('group_rows', 0) or 0), chunk_bytes=int(args.get('chunk_bytes', 0) or 0))
    except abi.MidasSnpsError as e:
        if getattr(e, 'linked', None) is not None:
            _exit("%d pairs of genes are linked, more than --max_pairs %d: raise --min_jaccard or --max_pairs"
                  % (e.linked, args['max_pairs']))
        genes_compare.exit_bad_row(matrix, e)
    finally:
        ctx.close()
    print("Rows read: %d" % res['n_rows'])
    print("Genes kept (present in >= %d and absent from >= %d of %d samples): %d"
          % (args['min_present'], args['min_absent'], n_samples, res['n_kept']))
    print("Pairs of genes visited: %d" % res['visited'])
    print("Linked pairs (Jaccard index >= %s): %d\n" % (repr(float(args['min_jaccard'])), res['linked']))
    sys.stdout.flush()
    try:
        matrix.write_linkage(args['out'], res)
        if args.get('groups'):
            res['n_groups'] = matrix.write_groups(args['groups'], res, int(args['min_group']))
            print("Groups of at least %d genes: %d\n" % (args['min_group'], res['n_groups']))
    except abi.MidasSnpsError as e:
        _exit(e.message)
    return res
