"""compare_genes.py on the GPU box: midas_genes_compare against the sequential model (tests/compare_genes_model.py) -- the
converted cells, every integer and every fp64 sum as bit patterns -- for all six modes at three group settings and at sample
counts around the pair tile; every golden case (tests/golden/compare_genes_vectors.json) in process and through the script; the
chain merge_midas.py genes -> compare_genes.py; and the earliest bad cell whatever the groups are."""
import os
import subprocess
import sys

import numpy as np
import pytest

from midas_amd import abi
from midas_amd import synth as reads_synth
from midas_amd.analyze import synth
from tests import compare_genes_model as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VEC = M.load_vectors()
CASES = list(range(len(VEC['cases'])))
MODES = [(t, d) for t in ('presabs', 'copynum') for d in ('jaccard', 'euclidean', 'manhattan')]
GROUPS = ((0, 0), (777, 60000), (50, 0))       # one group; not a multiple of 64, small chunks; fewer rows than a word


@pytest.fixture(scope="module")
def ctx():
    with abi.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return M.write_tree(str(tmp_path_factory.mktemp("compare_genes_gpu")), VEC)


def _matrix(tmp_path_factory, n_genes, n_samples, seed):
    d = str(tmp_path_factory.mktemp("genes") / "species_1")
    synth.write_genes_dir(d, n_genes, n_samples, seed=seed, block=3000)
    return abi.GenesMatrix(os.path.join(d, 'genes_copynum.txt'))


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _check(got, exp, dtype, distance, what):
    if dtype == 'presabs':
        assert np.array_equal(np.triu(got['count']), exp['count']), what
        return
    assert _same_bits(np.triu(got['both']), np.triu(exp['both'])), what
    assert _same_bits(np.triu(got['either']), np.triu(exp['either'])), what
    if distance != 'jaccard':
        assert _same_bits(np.triu(got['dist']), np.triu(exp['dist'])), what


def test_the_device_equals_the_model_bit_for_bit_at_every_group_setting(ctx, tmp_path_factory):
    n_genes, n_samples = 3333, 13                  # 3333 = 104 staging runs of 32 and 5 genes
    m = _matrix(tmp_path_factory, n_genes, n_samples, seed=5)
    cells, col_float = M.read_cells(m.text, n_genes, 11, n_samples)
    assert (cells != np.array([[float(c) for c in line.split(b'\t')[1:12]] for line in m.text.tobytes().split(b'\n')[:-1]]).T).mean() > 0.1
    for dtype, distance in MODES:
        exp = M.compare(cells, dtype, distance, 0.35)
        groups = []
        for group_rows, chunk in GROUPS:
            got = ctx.genes_compare(m.text, n_genes, 11, n_samples, dtype=dtype, distance=distance, cutoff=0.35, group_rows=group_rows,
                                    chunk_bytes=chunk, dump=True)
            assert got['n_rows'] == n_genes and _same_bits(got['cells'], cells), (dtype, distance, group_rows)
            assert np.array_equal(got['col_float'], col_float.astype(np.uint8))
            _check(got, exp, dtype, distance, (dtype, distance, group_rows))
            groups.append(got['groups'])
        assert groups[0] == 1 and groups[1] > 1 and groups[2] > groups[1], groups
    # rows beyond n_rows are not read
    got = ctx.genes_compare(m.text, 1000, 11, n_samples, dtype='copynum', distance='euclidean', group_rows=333)
    _check(got, M.compare(cells[:, :1000], 'copynum', 'euclidean', 0.35), 'copynum', 'euclidean', 'max_genes')
    assert got['n_rows'] == 1000


@pytest.mark.parametrize("n_samples", [2, 63, 64, 65, 130])
def test_sample_counts_around_the_pair_tile(ctx, tmp_path_factory, n_samples):
    n_genes = 403                                  # ends mid staging run
    m = _matrix(tmp_path_factory, n_genes, n_samples, seed=n_samples)
    cells, _ = M.read_cells(m.text, n_genes, n_samples, n_samples)
    for dtype, distance in MODES:
        exp = M.compare(cells, dtype, distance, 0.75)
        for group_rows in (0, 100):
            got = ctx.genes_compare(m.text, n_genes, n_samples, n_samples, dtype=dtype, distance=distance, cutoff=0.75, group_rows=group_rows)
            _check(got, exp, dtype, distance, (n_samples, dtype, distance, group_rows))
            assert got['tiles'] == (1 if n_samples <= 64 else 3 if n_samples <= 128 else 6)


@pytest.mark.parametrize("k", CASES)
def test_golden_cases_in_process(tree, tmp_path, k):
    case = VEC['cases'][k]
    for extra in ([], ['--group_rows', '37']):
        printed, table = M.run(tree[case['dir']], case['options'], str(tmp_path / 'out.txt'), _context, extra)
        assert table == M.case_table(case), extra
        assert printed == case['printed']


def _context():
    return abi.Context(0)


@pytest.mark.parametrize("k", CASES)
def test_golden_cases_through_the_script(tree, tmp_path, k):
    case = VEC['cases'][k]
    out = str(tmp_path / 'out.txt')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'compare_genes.py'), tree[case['dir']], '--out', out] + case['options'],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert open(out).read() == M.case_table(case) and r.stdout == case['printed']


def test_the_table_goes_to_stdout_after_the_progress_lines(tree):
    case = VEC['cases'][0]
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'compare_genes.py'), tree[case['dir']]] + case['options'],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert r.stdout == case['printed'] + M.case_table(case)


def test_the_earliest_bad_cell_is_reported_whatever_the_groups_are(ctx, tmp_path):
    rows = [r.split('\t') for r in VEC['dirs']['six'].split('\n')[:-1]]
    rows[100][2] = 'NA'
    rows[80].append('1.0')
    rows[50][5] = 'inf'
    rows[50][3] = ''
    d = M.write_dir(str(tmp_path / 'bad'), '\n'.join('\t'.join(r) for r in rows) + '\n')
    m = abi.GenesMatrix(os.path.join(d, 'genes_copynum.txt'))
    for group_rows, chunk in ((0, 0), (40, 0), (7, 2048), (49, 0), (50, 0)):
        for dtype in ('presabs', 'copynum'):
            with pytest.raises(abi.MidasSnpsError) as ei:
                ctx.genes_compare(m.text, m.n_rows, 6, 6, dtype=dtype, group_rows=group_rows, chunk_bytes=chunk)
            assert ei.value.status == abi.ERR_BAD_LAYOUT and ei.value.bad == (2, 49, 2), (group_rows, ei.value.bad)
    with pytest.raises(abi.MidasSnpsError) as ei:
        ctx.genes_compare(m.text, m.n_rows, 2, 6, group_rows=64)           # the bad cells are in no column in use: the width is
    assert ei.value.bad == (1, 79, -1)
    got = ctx.genes_compare(m.text, 49, 6, 6, group_rows=32)                # nor is a row beyond max_genes
    assert got['n_rows'] == 49
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'compare_genes.py'), d, '--out', str(tmp_path / 'o.txt')],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 1 and "genes_copynum.txt, line 51, column 4 (sample s002): the cell is not a finite decimal number" in r.stderr


WALKS = M.walker_cases()


@pytest.mark.parametrize("k", range(len(WALKS)), ids=[w[0] for w in WALKS])
def test_the_walk_of_the_rows_at_its_borders(ctx, k):
    name, body, n_rows, group_rows, chunk = WALKS[k]
    walk = M.walk(body, n_rows, group_rows, chunk)
    assert walk[0] == n_rows and (name != 'grow' or walk[3] == 128) and (group_rows != 1 or walk[1] == n_rows)
    cells, col_float = M.read_cells(body, n_rows, 6, 6)
    for dtype, distance in (('presabs', 'jaccard'), ('copynum', 'euclidean')):
        got = ctx.genes_compare(body, n_rows, 6, 6, dtype=dtype, distance=distance, group_rows=group_rows, chunk_bytes=chunk, dump=True)
        assert (got['n_rows'], got['groups'], got['group_rows'], got['chunk_bytes']) == walk, name
        assert _same_bits(got['cells'], cells) and np.array_equal(got['col_float'], col_float.astype(np.uint8)), name
        _check(got, M.compare(cells, dtype, distance, 0.35), dtype, distance, name)


@pytest.mark.parametrize("group_rows,chunk", [(10, 0), (1, 0), (0, 0), (10, 64)])
def test_a_short_row_in_one_group_wins_over_a_bad_cell_in_the_next(ctx, group_rows, chunk):
    body, bad = M.walker_bad_body()
    for dtype in ('presabs', 'copynum'):
        with pytest.raises(abi.MidasSnpsError) as ei:
            ctx.genes_compare(body, 30, 6, 6, dtype=dtype, group_rows=group_rows, chunk_bytes=chunk)
        assert ei.value.status == abi.ERR_BAD_LAYOUT and ei.value.bad == bad


def _write_gene_info(db, ds):
    for sp in ds['species_ids']:
        genes = [g for g, s in zip(ds['gene_ids'], ds['gene_species']) if s == sp]
        with open(os.path.join(db, 'pan_genomes', sp, 'gene_info.txt'), 'w') as h:
            h.write('gene_id\tgenome_id\tcentroid_99\tcentroid_95\tcentroid_90\tcentroid_85\tcentroid_80\tcentroid_75\n')
            for k, g in enumerate(genes):
                h.write('%s\t%s.rep\t%s\t%s\t%s\t%s\t%s\t%s\n' % (g, sp, g, genes[k - k % 2], genes[k - k % 3], genes[k - k % 4],
                                                                genes[k - k % 5], genes[0]))


def test_merge_midas_genes_then_compare_genes_chain(tmp_path):
    ds = reads_synth.make_pangenome_dataset(n_species=2, genes_per_species=60, n_reads=12000, seed=31)
    db = str(tmp_path / 'db')
    fq = str(tmp_path / 'reads.fq')
    with open(fq, 'w') as h:
        h.write("@r1\nACGT\n+\nIIII\n")
    rng = np.random.default_rng(3)
    dirs = []
    for k in range(3):
        idx = np.sort(rng.choice(ds['refid'].size, ds['refid'].size * (k + 2) // 5, replace=False))
        part = dict(ds, reads=reads_synth.take_reads(ds['reads'], idx), refid=ds['refid'][idx])
        d = str(tmp_path / ('sample_%d' % k))
        reads_synth.write_pangenome_sample(d, db, part)
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'run_midas.py'), 'genes', d, '--call_genes', '-d', db, '-1', fq],
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        dirs.append(d)
    _write_gene_info(db, ds)
    out = str(tmp_path / 'out')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'merge_midas.py'), 'genes', out, '-i', ','.join(dirs), '-t', 'list', '-d', db,
                        '--sample_depth', '0', '--min_copy', '0.5'], capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr
    for sp in ds['species_ids']:
        text = open(os.path.join(out, sp, 'genes_copynum.txt')).read()
        assert text.count('\n') > 10
        for dtype, distance in MODES:
            options = ['--dtype', dtype, '--distance', distance]
            dist = str(tmp_path / 'dist.txt')
            r = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'compare_genes.py'), os.path.join(out, sp), '--out', dist] + options,
                               capture_output=True, text=True, timeout=600)
            assert r.returncode == 0, r.stderr
            assert open(dist).read() == M.model_table(text, M.case_options(dict(options=options))), (sp, options)


# ---- gc_parse_kernel's converter (pandas_f64.h as device code) on the cells the host build alone has seen ------------------------------
from tests.test_compare_genes_host import EDGE, NOT_NUMBERS                           # noqa: E402


def _body(rows, eol='\n'):
    return np.frombuffer(''.join('g%d\t%s%s' % (r, '\t'.join(row), eol) for r, row in enumerate(rows)).encode(), np.uint8)


def test_edge_cells_on_the_device_are_the_models_bit_for_bit(ctx):
    """Every EDGE cell as the first, a middle and the last cell of a row: 1e-400 and 4.9e-324, the two-step division below
    1e-308 (a division with a subnormal quotient), 24-digit cells, padded cells, with \\n and with \\r\\n row ends."""
    S = 3
    rows = [[cell if c == at else ('1.5', '2', '7e-1')[(k + c) % 3] for c in range(S)] for k, cell in enumerate(EDGE) for at in range(S)]
    exp, col_float = M.read_cells(_body(rows), len(rows), S, S)
    assert (exp == 0).any() and (np.abs(exp[exp != 0]) < 2.3e-308).any() and col_float.all()
    for eol in ('\n', '\r\n'):
        for group_rows, chunk in GROUPS + ((7, 256),):
            got = ctx.genes_compare(_body(rows, eol), len(rows), S, S, group_rows=group_rows, chunk_bytes=chunk, dump=True)
            assert got['n_rows'] == len(rows)
            wrong = np.argwhere(got['cells'].view(np.uint64) != exp.view(np.uint64))
            assert wrong.shape[0] == 0, (eol, group_rows, [rows[r][c] for c, r in wrong.tolist()])
            assert np.array_equal(got['col_float'], col_float.astype(np.uint8))
    # a column of plain integers stays one
    ints = [['3', '1.5', '-12'], [' 4', '2', '7']]
    got = ctx.genes_compare(_body(ints), 2, S, S, dump=True)
    assert got['col_float'].tolist() == M.read_cells(_body(ints), 2, S, S)[1].astype(np.uint8).tolist() == [0, 1, 0]


@pytest.mark.parametrize("eol", ['\n', '\r\n'])
def test_cells_that_are_no_number_are_refused_with_their_place_on_the_device(ctx, eol):
    S, N = 3, 5
    for k, cell in enumerate(NOT_NUMBERS):
        for at in range(S):
            rows = [['1.5', '2', '0.25'] for _ in range(N)]
            r = (k + at) % N
            rows[r][at] = cell
            with pytest.raises(M.BadMatrix) as em:
                M.read_cells(_body(rows, eol), N, S, S)
            assert em.value.bad == (2, r, at)
            with pytest.raises(abi.MidasSnpsError) as ei:
                ctx.genes_compare(_body(rows, eol), N, S, S, group_rows=(0, 2)[k % 2])
            assert ei.value.status == abi.ERR_BAD_LAYOUT and ei.value.bad == (2, r, at), (cell, at, eol)
