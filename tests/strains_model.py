"""A sequential Python model of Context.sites_id_markers and Context.sites_track_markers (midas_sites_id_markers,
midas_sites_track_markers): the same arguments, the same outputs, every call formed the way the interpreter forms it -- sets
of samples per letter, sets of sites per sample, round().  The host tests inject it in place of the device; the GPU tests
compare the device calls with it, every integer.  It is written from the reference's loop (midas/analyze/track_strains.py),
not from the kernels."""
import base64
import json
import lzma
import os

import numpy as np

from tests import analyze_model as A

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "strain_vectors.json")


def load_vectors():
    with open(GOLDEN) as f:
        return json.load(f)


def expected_out(case):
    """The output file the reference wrote for a golden case (a large one is kept as base64 of its xz stream)."""
    return case['out'] if 'out' in case else lzma.decompress(base64.b64decode(case['out_xz'])).decode()


class _Cells:
    """float() / int() of the selected samples' cells, a row at a time as the reference's loop converts them: iterating yields
    (row, f [sample], d [sample]) for the first n_parse rows; .side counts the cells off the device's fast path."""

    def __init__(self, freq_text, depth_text, sample_col, n_parse):
        self.frows, self.drows = A._rows(freq_text), A._rows(depth_text)
        self.cols = [int(c) for c in sample_col]
        self.n = min(int(n_parse), len(self.frows), len(self.drows))
        self.side = [0, 0]

    def __iter__(self):
        for i in range(self.n):
            f, d = [], []
            for s, c in enumerate(self.cols):
                for m, (row, fast, out) in enumerate(((self.frows[i][1:], A.is_fast_float, f), (self.drows[i][1:], A.is_fast_int, d))):
                    if c >= len(row):
                        raise A.BadCell((m + 1, i, -1), "data row %d: fewer columns than the samples in use" % i)
                    self.side[m] += not fast(row[c])
                    v = A.abi_parse(row[c], m)
                    if v is None:
                        raise A.BadCell((m + 1, i, s), "data row %d, sample %d: not a number" % (i, s))
                    out.append(v)
            yield i, f, d


def _round(x, i, s):
    try:
        return round(x)
    except (OverflowError, ValueError):
        raise A.BadCell((3, i, s), "data row %d, sample %d: frequency x depth is not a finite number" % (i, s))


def sites_id_markers(freq_text, depth_text, minor_code, major_code, sample_col, min_freq, min_reads, allele_prev, n_parse=None,
                     group_rows=0, chunk_bytes=0):
    n_call = len(minor_code)
    cells = _Cells(freq_text, depth_text, sample_col, n_call if n_parse is None else n_parse)
    rows = []
    for i, F, D in cells:
        if i >= n_call:
            continue
        mi, ma = int(minor_code[i]), int(major_code[i])
        groups = [set(), set(), set(), set()]
        total = set()
        for s, (f, d) in enumerate(zip(F, D)):
            if d == 0:
                continue
            if f >= min_freq and _round(f * d, i, s) >= min_reads:
                if mi > 3:
                    raise A.BadCell((4, i, s), "data row %d, sample %d: the minor allele is none of A, T, C, G" % (i, s))
                groups[mi].add(s)
            if (1 - f) >= min_freq and _round((1 - f) * d, i, s) >= min_reads:
                if ma > 3:
                    raise A.BadCell((5, i, s), "data row %d, sample %d: the major allele is none of A, T, C, G" % (i, s))
                groups[ma].add(s)
            total.add(s)
        counts = [len(g) for g in groups]
        alleles = sorted([(k, c) for k, c in enumerate(counts) if c > 0], key=lambda kc: kc[1])
        if len(alleles) != 2 or alleles[0][1] > allele_prev:
            continue
        rows.append([i, alleles[0][0], len(total)] + counts)
    return dict(rows=np.array(rows, np.int32).reshape(-1, 7), n_sites=cells.n, groups=1, side_freq=cells.side[0], side_depth=cells.side[1], ms=[0.0] * 8)


def sites_track_markers(freq_text, depth_text, site_which, sample_col, min_freq, min_reads, n_parse=None, group_rows=0, chunk_bytes=0,
                        pair_blocks=0):
    n_call = len(site_which)
    S = len(sample_col)
    cells = _Cells(freq_text, depth_text, sample_col, n_call if n_parse is None else n_parse)
    markers = [set() for _ in range(S)]
    matched = 0
    for i, F, D in cells:
        if i >= n_call or not site_which[i]:
            continue
        matched += 1
        for s, (f, d) in enumerate(zip(F, D)):
            if d == 0:
                continue
            mf = 1 - f if site_which[i] == 1 else f
            count = _round(mf * d, i, s)
            if mf >= min_freq and count >= min_reads:
                markers[s].add(i)
    both = np.zeros((S, S), np.int64)
    for a in range(S):
        for b in range(a, S):
            both[a, b] = len(markers[a] & markers[b])
    return dict(both=both, n_matched=matched, n_sites=cells.n, groups=1, side_freq=cells.side[0], side_depth=cells.side[1], ms=[0.0] * 8)


class ModelContext:
    """Stands in for abi.Context in strains.id_markers / strains.track_markers."""

    def sites_id_markers(self, *a, **kw):
        return sites_id_markers(*a, **kw)

    def sites_track_markers(self, *a, **kw):
        return sites_track_markers(*a, **kw)

    def close(self):
        pass


# ---- what the host tests and the GPU tests share: the golden tree and a command run in process ----------------------------------
def write_species(d, sp):
    os.makedirs(d, exist_ok=True)
    for k in ('summary', 'info', 'freq', 'depth'):
        with open('%s/snps_%s.txt' % (d, k), 'w', newline='') as f:
            f.write(sp[k])


def write_tree(tmp, vec):
    """The golden species and marker lists as files under tmp."""
    for name, sp in vec['species'].items():
        write_species('%s/%s' % (tmp, name), sp)
    for name, text in vec['markers'].items():
        with open('%s/%s.txt' % (tmp, name), 'w') as f:
            f.write(text)
    return tmp


def argv_of(tree, program, case, out, marker_names=()):
    return [program, '--indir', '%s/%s' % (tree, case['species']), '--out', out] + \
        ['%s/%s.txt' % (tree, o) if o in marker_names else o for o in case['options']]


def run(tree, program, case, out, make_context=ModelContext, extra=(), marker_names=()):
    """The command in this process -> (parsed arguments, what it printed)."""
    import contextlib
    import io
    from midas_amd.analyze import cli, strains
    parse, pipeline = (cli.id_markers_arguments, strains.id_markers) if program == 'id_markers' else \
        (cli.track_markers_arguments, strains.track_markers)
    args = parse(argv_of(tree, program, case, out, marker_names) + list(extra))
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        pipeline(args, make_context=make_context)
    return args, buf.getvalue()


def check_case(tree, program, case, out, make_context=ModelContext, extra=(), marker_names=()):
    """A golden case: the output file's bytes, the printed lines and the parsed arguments are the reference's."""
    args, printed = run(tree, program, case, out, make_context, extra, marker_names)
    with open(out, newline='') as f:
        assert f.read() == expected_out(case)
    assert printed == case['printed']
    for k, v in case['args'].items():              # the reference's parser on the same command line
        exp = v.replace('<TMP>', tree).replace('%s/out.txt' % tree, out) if isinstance(v, str) else v
        assert args[k] == exp, k
