"""The sequential model of compare_genes.py: the cell converter of pandas' C reader, the presence / absence calls, the ordered
fp64 sums and str() of every number -- plain Python and numpy, no device.  ModelContext stands in for abi.Context in the
host tests (make_context=); the GPU tests compare the device with compare() bit for bit."""
import itertools
import math

import numpy as np

from midas_amd import abi

POW10 = [float('1e%d' % k) for k in range(309)]       # correctly rounded, as the reader's table


def _space(c):
    return c == ' ' or '\t' <= c <= '\r'


def pandas_float(cell):
    """-> (value, plain_int) as read_table converts the cell under its default float_precision, or None when the cell is no
    finite decimal literal.  At most 17 digits go into number = number * 10.0 + digit; then ONE multiply or divide."""
    s, n, i = cell, len(cell), 0
    while i < n and _space(s[i]):
        i += 1
    neg = False
    if i < n and s[i] in '+-':
        neg = s[i] == '-'
        i += 1
    number, exponent, digits, decimals, seen, plain = 0.0, 0, 0, 0, False, True
    while i < n and '0' <= s[i] <= '9':
        seen = True
        if digits < 17:
            number = number * 10.0 + float(ord(s[i]) - 48)
            digits += 1
        else:
            exponent += 1
        i += 1
    if i < n and s[i] == '.':
        plain = False
        i += 1
        while i < n and '0' <= s[i] <= '9':
            seen = True
            if digits < 17:
                number = number * 10.0 + float(ord(s[i]) - 48)
                digits += 1
                decimals += 1
            i += 1
        exponent -= decimals
    if not seen:
        return None
    if neg:
        number = -number
    if i < n and s[i] in 'eE':
        plain = False
        i += 1
        eneg = False
        if i < n and s[i] in '+-':
            eneg = s[i] == '-'
            i += 1
        j = i
        while i < n and '0' <= s[i] <= '9':
            i += 1
        if i == j:
            return None
        e10 = min(int(s[j:i]), 100000)
        exponent += -e10 if eneg else e10
    while i < n and _space(s[i]):
        i += 1
    if i != n or exponent > 308:
        return None
    if exponent > 0:
        number = number * POW10[exponent]
    elif exponent < -616:
        number = 0.0
    elif exponent < -308:
        number = number / POW10[-308 - exponent] / POW10[308]
    else:
        number = number / POW10[-exponent]
    if math.isinf(number):
        return None
    return number, plain


class BadMatrix(Exception):
    """kind 1: a row of another width, 2: a cell; data row, sample column (-1 for the width)."""

    def __init__(self, kind, row, col):
        Exception.__init__(self, "kind %d, data row %d, column %d" % (kind, row, col))
        self.bad = (kind, row, col)


def read_cells(text, n_rows, n_samples, n_columns):
    """The first n_samples columns of rows [0, n_rows) of the body text -> (cells f64 [S, rows], col_float bool [S]); the
    earliest bad row or cell in file order raises BadMatrix."""
    if isinstance(text, np.ndarray):
        text = text.tobytes()
    if isinstance(text, bytes):
        text = text.decode('utf-8', errors='surrogateescape')
    lines = text.split('\n')
    if lines and lines[-1] == '':
        lines.pop()
    lines = lines[:n_rows]
    cells = np.zeros((n_samples, len(lines)), np.float64)
    col_float = np.zeros(n_samples, bool)
    for r, line in enumerate(lines):
        if line.endswith('\r'):
            line = line[:-1]
        f = line.split('\t')[1:]
        if len(f) != n_columns:
            raise BadMatrix(1, r, -1)
        for c in range(n_samples):
            v = pandas_float(f[c])
            if v is None:
                raise BadMatrix(2, r, c)
            cells[c, r] = v[0]
            col_float[c] |= not v[1]
    return cells, col_float


def walk(text, n_rows, group_rows, chunk_bytes):
    """The walk of rows [0, n_rows) of a body of less than 1 MiB by row groups, as the statistics report it -> (rows read,
    groups, group_rows, chunk_bytes).  A chunk is the next chunk_bytes bytes (at least 64, at most the body and one byte; 0:
    that), a final line without '\\n' gets one; a group is the chunk's complete lines, at most group_rows (0: n_rows) of them;
    a chunk without a complete line is doubled."""
    text = text.tobytes() if isinstance(text, np.ndarray) else text
    n = len(text)
    cb = min(max(chunk_bytes if chunk_bytes else 1 << 20, 64), max(64, n + 1))
    G = max(1, min(group_rows if group_rows else n_rows, n_rows, cb))
    at = base = groups = 0
    while base < n_rows:
        chunk = text[at:at + cb]
        eof = at + len(chunk) == n
        if eof and chunk and not chunk.endswith(b'\n'):
            chunk += b'\n'
        ends = [k for k, c in enumerate(chunk) if c == 10]
        g = min(len(ends), G, n_rows - base)
        if g == 0:
            if eof:
                break
            cb *= 2
            continue
        groups += 1
        base += g
        at = min(n, at + ends[g - 1] + 1)
    return base, groups, G, cb


def walker_cases():
    """The borders of the walk on 50 rows of 6 samples, row 20 longer than 64 bytes -> [(name, body uint8, n_rows, group_rows,
    chunk_bytes)]: a chunk that must grow, a last line without '\\n', CRLF, fewer rows asked for than the file has, groups of
    one row."""
    rng = np.random.default_rng(3)
    spell = ('1.5', '0.36', '0.0', '0.35', '12', '7e-1', '0', '3.4e-1')
    rows = [['g%d' % r] + [spell[k] for k in rng.integers(0, len(spell), 6)] for r in range(50)]
    rows[20][1:] = ['1.50000000000000000', '0.00000000000000000', '0.36000000000000000', '0.0', '12.0000000000000000', '0.35']
    assert len('\t'.join(rows[20])) > 64 and max(len('\t'.join(r)) for r in rows[:20] + rows[21:]) < 40

    def body(eol='\n', last=True):
        t = eol.join('\t'.join(r) for r in rows) + (eol if last else '')
        return np.frombuffer(t.encode(), np.uint8)
    return [('grow', body(), 50, 7, 64), ('no last newline', body(last=False), 50, 7, 256), ('no last newline, one group', body(last=False), 50, 0, 0),
            ('crlf', body('\r\n'), 50, 7, 256), ('crlf, no last newline', body('\r\n', False), 50, 0, 100), ('fewer rows', body(), 33, 10, 200),
            ('fewer rows, one group', body(), 33, 0, 0), ('one row a group', body(), 50, 1, 0), ('one row a group, grow', body(), 50, 1, 64)]


def walker_bad_body():
    """Row 5 is short and row 15 holds a cell that is no number: with groups of 10 rows the short row is the first group's and
    must win -> (body, .bad)."""
    rows = [['g%d' % r, '1.5', '0.0', '0.36', '0', '12', '0.35'] for r in range(30)]
    rows[5].pop()
    rows[15][2] = 'NA'
    return np.frombuffer(('\n'.join('\t'.join(r) for r in rows) + '\n').encode(), np.uint8), (1, 5, -1)


def ordered_sum(x):
    """sum() of the rows of x [rows, ...] front to back, one fp64 add each (numpy's cumsum adds sequentially; the host test
    checks that against Python's sum)."""
    x = np.asarray(x, np.float64)
    if x.shape[0] == 0:
        return np.zeros(x.shape[1:], np.float64)
    return np.cumsum(x, axis=0)[-1]


def compare(cells, dtype, distance, cutoff):
    """-> dict of [S, S] arrays filled for i <= j, as Context.genes_compare returns them."""
    S, G = cells.shape
    out = dict(count=None, both=None, either=None, dist=None)
    if dtype == 'presabs':
        p = (cells > cutoff).astype(np.int64)
        out['count'] = np.triu(p @ p.T)
        return out
    both, either = np.zeros((S, S)), np.zeros((S, S))
    dist = np.zeros((S, S)) if distance != 'jaccard' else None
    for i in range(S):
        a = cells[i][:, None]                      # [G, 1]
        b = cells[i:].T                            # [G, S - i]
        both[i, i:] = ordered_sum(np.where(b < a, b, a))
        either[i, i:] = ordered_sum(np.where(b > a, b, a))
        if distance == 'euclidean':
            d = a - b
            dist[i, i:] = ordered_sum(d * d)
        elif distance == 'manhattan':
            dist[i, i:] = ordered_sum(np.abs(a - b))
    out.update(both=both, either=either, dist=dist)
    return out


def table_text(ids, res, dtype, distance, n_rows):
    """The output table from compare()'s arrays, every number as str() writes it."""
    rows = ['\t'.join(['sample1', 'sample2', 'count1', 'count2', 'count_both', 'count_either', 'distance'])]
    for i, j in itertools.combinations(range(len(ids)), 2):
        if dtype == 'presabs':
            c = res['count']
            c1, c2, b = int(c[i, i]), int(c[j, j]), int(c[i, j])
            u = c1 + c2 - b
            if distance == 'jaccard':
                d = 1 - (float(b) / u) if u > 0 else 0
            elif distance == 'euclidean':
                d = math.sqrt(c1 + c2 - 2 * b)
            else:
                d = float(c1 + c2 - 2 * b)
        elif n_rows == 0:
            c1 = c2 = b = u = 0
            d = 0 if distance == 'jaccard' else 0.0
        else:
            c1 = c2 = float(res['both'][j, j])
            b, u = float(res['both'][i, j]), float(res['either'][i, j])
            if distance == 'jaccard':
                d = 1 - (b / u) if u > 0 else 0
            elif distance == 'euclidean':
                d = math.sqrt(float(res['dist'][i, j]))
            else:
                d = float(res['dist'][i, j])
        rows.append('\t'.join(str(v) for v in [ids[i], ids[j], c1, c2, b, u, d]))
    return '\n'.join(rows) + '\n'


def model_table(matrix_text, options):
    """The whole command over the text of genes_copynum.txt -> the output table."""
    header, _, body = matrix_text.partition('\n')
    ids = header.split('\t')[1:]
    n_rows = body.count('\n') + (1 if body and not body.endswith('\n') else 0)
    if options.get('max_genes') is not None:
        n_rows = min(n_rows, options['max_genes'])
    S = options.get('max_samples') or len(ids)
    cells, _ = read_cells(body, n_rows, S, len(ids))
    dtype, distance = options.get('dtype', 'presabs'), options.get('distance', 'jaccard')
    return table_text(ids[:S], compare(cells, dtype, distance, options.get('cutoff', 0.35)), dtype, distance, cells.shape[1])


class ModelContext:
    """A CPU double of abi.Context for midas_amd.analyze.genes_compare: the same call, the same result keys, the same error."""

    def genes_compare(self, text, n_rows, n_samples, n_columns, dtype='presabs', distance='jaccard', cutoff=0.35, group_rows=0,
                      chunk_bytes=0, pair_blocks=0, dump=False):
        try:
            cells, col_float = read_cells(text, n_rows, n_samples, n_columns)
        except BadMatrix as b:
            e = abi.MidasSnpsError(abi.ERR_BAD_LAYOUT, str(b))
            e.bad = b.bad
            raise e
        out = compare(cells, dtype, distance, cutoff)
        out.update(dtype=dtype, distance=distance, n_samples=n_samples, n_rows=cells.shape[1], col_float=col_float.astype(np.uint8), groups=1)
        if dump:
            out['cells'] = cells
        return out

    def close(self):
        pass


# ---- the golden vectors (tests/golden/compare_genes_vectors.json) and runs of the host module over them -----------------------
def load_vectors():
    import base64
    import json
    import lzma
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'compare_genes_vectors.json')) as h:
        vec = json.load(h)
    for name, packed in vec.pop('dirs_xz', {}).items():
        vec['dirs'][name] = lzma.decompress(base64.b64decode(packed)).decode()
    return vec


def case_table(case):
    import base64
    import lzma
    return case['out'] if 'out' in case else lzma.decompress(base64.b64decode(case['out_xz'])).decode()


def case_options(case):
    """The options of a golden case as model_table takes them."""
    o, it = {}, iter(case['options'])
    for a in it:
        v = next(it)
        o[a[2:]] = v if a in ('--dtype', '--distance') else float(v) if a == '--cutoff' else int(v)
    return o


def write_dir(d, copynum_text):
    import os
    os.makedirs(d, exist_ok=True)
    for kind in ('presabs', 'depth'):
        open('%s/genes_%s.txt' % (d, kind), 'w').close()
    with open('%s/genes_copynum.txt' % d, 'w', newline='') as f:
        f.write(copynum_text)
    return d


def write_tree(root, vec):
    import os
    return {name: write_dir(os.path.join(root, name), text) for name, text in vec['dirs'].items()}


def run(indir, options, out, make_context, extra=()):
    """compare_genes.py in process -> (what it printed, the table it wrote)."""
    import contextlib
    import io
    from midas_amd.analyze import cli, genes_compare
    args = cli.compare_genes_arguments([indir, '--out', out] + list(options) + list(extra))
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        genes_compare.compare(args, make_context=make_context)
    with open(out) as f:
        return buf.getvalue(), f.read()
