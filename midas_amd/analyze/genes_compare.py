"""MI355X-native compare_genes.py: the host side.

Mirrors the reference's scripts/compare_genes.py (everything there is under __main__).  Only genes_copynum.txt is read; it is
mapped and handed to the device as text.  One device call converts the cells the way pandas' reader does, calls presence /
absence or forms the ordered fp64 sums for every pair of samples; the pair table is written natively.

Where the reference leans on a pandas quirk this build ends with an error of its own that names file, line and column
(DESIGN.md lists them): a first header field other than gene_id, --max_samples beyond the columns, a duplicated sample id, a
row of another width, a cell that is no finite decimal literal, and under --dtype copynum a column without a '.' or an exponent
in any cell (pandas would make it int64 and the printed sums would lose their '.0').
"""
import os
import sys

from midas_amd import abi
from midas_amd.analyze import sites as S


def _exit(message):
    sys.exit("\nError: %s\n" % message)


def open_matrix(path):
    try:
        return abi.GenesMatrix(path)
    except abi.MidasSnpsError as e:
        _exit(e.message)


def select(matrix, max_genes, max_samples):
    """-> (rows to read, sample columns to use): nrows=max_genes (None: all, 0: none), usecols=range(max_samples + 1) (0 or
    None: all)."""
    if matrix.first_field != 'gene_id':
        _exit("%s, line 1: the first column is '%s', not gene_id" % (matrix.path, matrix.first_field))
    if max_genes is not None and max_genes < 0:
        _exit("--max_genes cannot be a negative number")
    if max_samples is not None and max_samples < 0:
        _exit("--max_samples cannot be a negative number")
    n_samples = max_samples or matrix.n_columns
    if n_samples > matrix.n_columns:
        _exit("%s, line 1: --max_samples %d, but the matrix has %d sample columns" % (matrix.path, n_samples, matrix.n_columns))
    if n_samples < 1:
        _exit("%s, line 1: the matrix has no sample column" % matrix.path)
    seen = {}
    for k, id in enumerate(matrix.sample_ids[:n_samples]):
        if id in seen:
            _exit("%s, line 1: the sample id %s names columns %d and %d" % (matrix.path, id, seen[id] + 2, k + 2))
        seen[id] = k
    n_rows = matrix.n_rows if max_genes is None else min(matrix.n_rows, max_genes)
    return n_rows, n_samples


def exit_bad_row(matrix, e):
    """Leaves with the message of a device call's error: its own, or the place of the row or cell that cannot be read."""
    bad = getattr(e, 'bad', None)
    if not bad:
        _exit(e.message)
    if bad[0] == 1:
        _exit("%s, line %d: the row does not have %d sample columns" % (matrix.path, bad[1] + 2, matrix.n_columns))
    _exit("%s, line %d, column %d (sample %s): the cell is not a finite decimal number"
          % (matrix.path, bad[1] + 2, bad[2] + 2, matrix.sample_ids[bad[2]]))


def compare(args, make_context=S.device_context):
    """The command.  make_context: tests substitute a CPU double of the device."""
    print("Reading gene copy-number matrix\n")
    matrix = open_matrix(args['copynum'])
    n_rows, n_samples = select(matrix, args['max_genes'], args['max_samples'])
    ctx = make_context()
    try:
        res = ctx.genes_compare(matrix.text, n_rows, n_samples, matrix.n_columns, dtype=args['dtype'], distance=args['distance'],
                                cutoff=float(args['cutoff']), group_rows=int(args.get('group_rows', 0) or 0),
                                chunk_bytes=int(args.get('chunk_bytes', 0) or 0))
    except abi.MidasSnpsError as e:
        exit_bad_row(matrix, e)
    finally:
        ctx.close()
    if args['dtype'] == 'presabs':
        print("Converting to gene presence-absence matrix\n")
    elif res['n_rows'] > 0:
        for k in range(n_samples):
            if not res['col_float'][k]:
                _exit("%s, column %d (sample %s): no cell has a decimal point or an exponent; --dtype copynum needs a column of "
                      "decimal numbers" % (matrix.path, k + 2, matrix.sample_ids[k]))
    print("Computing distances between sample pairs\n")
    sys.stdout.flush()
    try:
        matrix.write_pairs(args['out'], res)
    except abi.MidasSnpsError as e:
        _exit(e.message)
    return res
