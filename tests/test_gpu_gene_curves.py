"""gene_curves.py on the GPU box: midas_genes_curves against the sequential model (tests/gene_curves_model.py), every output
array equal and int64 -- at sample counts around the 64-step word and around each width of the counter planes (7, 10, 13), at
gene counts around the 64-gene word, the 4 096 genes of a wave and the 16 384 genes of a workgroup, past the 2 048 steps a
workgroup keeps in LDS, with a column that is in no order, at three group settings and in both forms; the borders of need[];
a soft core that comes back; broken orders; a malformed cell; the script and the chain merge_midas.py genes -> gene_curves.py."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from midas_amd import abi
from midas_amd.analyze import genes_curves, synth
from tests import compare_genes_model as CG
from tests import gene_curves_model as M
from tests.test_gpu_compare_genes import _write_gene_info
from tests.test_gpu_gene_linkage import ABSENT, GROUPS, PRESENT, _body, _case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPT = os.path.join(ROOT, 'scripts', 'gene_curves.py')
ARRAYS = ('pan', 'core', 'single')
LEVELS = (1.0, 1.0, 0.97, 0.7, 0.3, 0.02)


@pytest.fixture(scope="module")
def ctx():
    with abi.Context(0) as c:
        yield c


def _text(present, seed=0):
    """test_gpu_gene_linkage._body for large matrices: the same spellings above and at or below the cutoff 0.35, picked by array."""
    rng = np.random.default_rng(seed)
    present = np.asarray(present, bool)
    pick = rng.integers(0, 5, present.shape)
    cells = np.where(present, np.array(PRESENT)[pick], np.array(ABSENT)[pick])
    return np.frombuffer(('\n'.join('g%d\t%s' % (g, '\t'.join(row)) for g, row in enumerate(cells.tolist())) + '\n').encode(), np.uint8)


def _mix(genes, S, seed, left_out=None):
    """A presence matrix [genes][S] of mixed prevalence (every sample, about 97, 70, 30 and 2 % of them); with left_out that column
    is set in every gene, gene 1 is present in that column alone, gene 2 nowhere, and the last gene in the first used column."""
    rng = np.random.default_rng(seed)
    present = rng.random((genes, S)) < np.array(LEVELS)[rng.integers(0, len(LEVELS), genes)][:, None]
    if left_out is not None:
        used = [s for s in range(S) if s != left_out]
        if genes >= 3:
            present[1] = False
            present[2] = False
        present[genes - 1, used[0]] = True
        present[:, left_out] = True
        if genes >= 3:
            present[2, left_out] = False
    return present


def _orders(used, R, seed):
    return genes_curves.orders_table(used, R - 1, seed)


def _expect(present, orders, need):
    return M.curves(np.asarray(present, np.float64).T, 0.35, orders, need)


def _same(got, exp, what):
    for k in ARRAYS:
        assert got[k].dtype == np.int64 and got[k].shape == exp[k].shape and np.array_equal(got[k], exp[k]), (what, k)


def _run(ctx, body, S, orders, need, exp, what):
    """Every group setting in both forms -> the six results, form 0 before form 1 at each setting."""
    n = int((body == 10).sum())
    seen = []
    for group_rows, chunk in GROUPS:
        for form in (0, 1):
            got = abi.genes_curves(ctx, body, n, S, S, orders, np.array(need, np.int32), form=form, group_rows=group_rows, chunk_bytes=chunk)
            assert got['n_rows'] == n and got['form'] == form and got['n_used'] == orders.shape[1] and got['n_orders'] == orders.shape[0]
            _same(got, exp, (what, group_rows, chunk, form))
            seen.append(got)
    return seen


def _not_trivial(exp):
    """A kernel that returns zeros, or the same curve for every order, cannot pass."""
    assert np.any((0 < exp['core']) & (exp['core'] < exp['pan'])) and exp['single'].max() > 0
    assert exp['pan'].shape[0] < 2 or any(not np.array_equal(exp[k][0], exp[k][1]) for k in ARRAYS)


@pytest.mark.parametrize("N", [1, 2, 63, 64, 65])
@pytest.mark.parametrize("genes", [1, 63, 64, 65, 130, 300])
def test_the_device_equals_the_model_around_the_word_of_genes_and_the_word_of_steps(ctx, N, genes):
    S, left_out = N + 1, N // 2
    used = [s for s in range(S) if s != left_out]
    present = _mix(genes, S, seed=1000 * N + genes, left_out=left_out)
    assert present[:, left_out].sum() >= genes - 1
    body = _body(present, seed=genes)
    cells, _ = CG.read_cells(body, genes, S, S)
    assert np.array_equal(cells > 0.35, present.T)
    orders = _orders(used, 4, seed=N)
    need = M.need_linear(N, 0.9)
    assert genes_curves.need_table(N, 0.9).tolist() == need
    exp = M.curves(cells, 0.35, orders, need)
    if genes >= 3:
        # gene 1 lives in the column no order holds and gene 2 nowhere: with them, pan never reaches the number of genes
        assert present[1].sum() == 1 and present[1, left_out] and not present[2].any() and exp['pan'].max() <= genes - 2
    assert present[genes - 1, used[0]]                       # the last word holds a set bit, and pad bits unless genes is a multiple of 64
    if N >= 63 and genes >= 63:
        _not_trivial(exp)
    seen = _run(ctx, body, S, orders, need, exp, (N, genes))
    assert seen[0]['groups'] == 1 and seen[0]['words'] == (genes + 63) // 64 and (genes <= 100 or seen[2]['groups'] > 1)
    assert seen[1]['planes'] == 7 and seen[0]['planes'] == 0


@pytest.mark.parametrize("N,planes", [(127, 7), (128, 10), (129, 10), (255, 10), (256, 10), (257, 10), (1023, 10), (1024, 13), (1025, 13),
                                      (4100, 13), (8191, 13)])
def test_the_counter_planes_at_both_sides_of_each_width(ctx, N, planes):
    """Gene 0 is present in all N samples: its count reaches N and the top plane in use carries at every power of two; gene 1
    in N - 1 and gene 2 in exactly one.  4 100 and 8 191 steps take three and four segments of the workgroup's LDS sums."""
    genes = 20 if N == 8191 else 70
    present = _mix(genes, N, seed=N)
    present[0] = True
    present[1] = True
    present[1, N // 3] = False
    present[2] = False
    present[2, N - 2] = True
    body = _text(present, seed=N)
    orders = _orders(range(N), 3, seed=N)
    need = genes_curves.need_table(N, 0.9).tolist()
    exp = _expect(present, orders, need)
    assert (exp['pan'][:, -1] == exp['pan'][0, -1]).all() and exp['core'].min() >= 1
    _not_trivial(exp)
    seen = _run(ctx, body, N, orders, need, exp, N)
    assert all(g['planes'] == (planes if g['form'] else 0) for g in seen)


@functools.lru_cache(maxsize=2)
def _chunk_case(genes, N):
    present = _mix(genes, N, seed=genes + N)
    present[genes - 1] = True
    return present, _text(present, seed=genes)


@pytest.mark.parametrize("R", [1, 2, 5])
@pytest.mark.parametrize("genes,N", [(g, N) for g in (4095, 4096, 4097, 8200) for N in (7, 70)] + [(16384, 7), (16385, 7)])
def test_gene_counts_around_a_wave_s_and_a_workgroup_s_words(ctx, genes, N, R):
    """A wave owns 64 words = 4 096 genes, a workgroup 256 words = 16 384 genes: one more gene is one more wave, one more
    workgroup.  R = 1 is --permutations 0."""
    present, body = _chunk_case(genes, N)
    need = genes_curves.need_table(N, 0.9).tolist()
    orders = _orders(range(N), R, seed=R)
    exp = _expect(present, orders, need)
    _not_trivial(exp)
    seen = _run(ctx, body, N, orders, need, exp, (genes, N, R))
    assert seen[0]['groups'] == 1 and seen[0]['words'] == (genes + 63) // 64 and seen[2]['groups'] > 1


def test_need_at_its_borders(ctx):
    N = 20
    need = genes_curves.need_table(N, 0.95).tolist()
    assert need[19] == 19 and need[20] == 19 and need == M.need_linear(N, 0.95)
    # one gene that misses sample 5 alone, under orders that add sample 5 first, 19th and last
    rest = [s for s in range(N) if s != 5]
    orders = np.array([list(range(N)), [5] + rest, rest[:18] + [5] + rest[18:], rest + [5]], np.int32)
    gene = np.ones((1, N), bool)
    gene[0, 5] = False
    # (the listed order adds it 6th: 5 of 6 up to 18 of 19 are too few, 19 of 20 are enough)
    curve = [[1] * 5 + [0] * 14 + [1], [0] * 19 + [1], [1] * 18 + [0, 1], [1] * 20]
    exp = _expect(gene, orders, need)
    assert exp['core'].tolist() == curve
    _run(ctx, _body(gene), N, orders, need, exp, 'one sample short')
    # among other genes the same orders
    present = _mix(200, N, seed=20)
    present[7] = gene[0]
    exp = _expect(present, orders, need)
    _not_trivial(exp)
    _run(ctx, _body(present), N, orders, need, exp, 'one sample short, among others')
    # at 0.75 six of eight are enough and five are not
    need = genes_curves.need_table(N, 0.75).tolist()
    assert need[8] == 6
    two = np.zeros((2, N), bool)
    two[0, [0, 1, 2, 4, 6, 7]] = True
    two[1, [0, 1, 2, 4, 6]] = True
    orders = _orders(range(N), 2, seed=1)
    exp = _expect(two, orders, need)
    assert exp['core'][0, 7] == 1 and exp['pan'][0, 7] == 2 and _expect(two[1:], orders, need)['core'][0, 7] == 0
    _run(ctx, _body(two), N, orders, need, exp, 'at need and one below')


def test_a_soft_core_gene_drops_out_and_comes_back(ctx):
    N = 8
    need = genes_curves.need_table(N, 0.75).tolist()
    assert need == [0, 1, 2, 3, 3, 4, 5, 6, 6]
    # counts 1 2 2 2 3 4 5 6 against need 1 2 3 3 4 5 6 6: core at k = 1, 2 and again at k = 8
    gene = np.array([[True, True, False, False, True, True, True, True]])
    orders = np.array([list(range(N)), [2, 3, 0, 1, 4, 5, 6, 7]], np.int32)
    assert _expect(gene, orders, need)['core'].tolist() == [[1, 1, 0, 0, 0, 0, 0, 1], [0, 0, 0, 0, 0, 0, 0, 1]]
    present = np.concatenate([np.repeat(gene, 40, axis=0), _mix(150, N, seed=8)])
    exp = _expect(present, orders, need)
    assert (np.diff(exp['core'][0]) > 0).any() and (np.diff(exp['core'][0]) < 0).any()
    _not_trivial(exp)
    _run(ctx, _body(present), N, orders, need, exp, 'soft core')


def test_a_core_of_every_sample(ctx):
    N = 70
    present = _mix(500, N, seed=70)
    need = genes_curves.need_table(N, 1.0).tolist()
    orders = _orders(range(N), 6, seed=6)
    exp = _expect(present, orders, need)
    _not_trivial(exp)
    everywhere = int(present.all(axis=1).sum())
    assert 0 < everywhere < 500
    for got in _run(ctx, _body(present), N, orders, need, exp, 'core_frac 1.0'):
        assert (got['core'][:, N - 1] == everywhere).all() and (np.diff(got['core'], axis=1) <= 0).all()
        assert (got['pan'][:, N - 1] == got['pan'][0, N - 1]).all() and (got['single'][:, N - 1] == got['single'][0, N - 1]).all()


def test_broken_orders_and_need_are_refused_before_the_device_and_leave_the_outputs_alone(ctx):
    S, N = 10, 8
    present = _mix(50, S, seed=3)
    body = _body(present)
    good = _orders(range(N), 3, seed=1)
    need = genes_curves.need_table(N, 0.9)

    def refused(orders, need, words):
        out = [np.full(orders.shape, -7, np.int64) for _ in range(3)]
        for form in (0, 1):
            with pytest.raises(abi.MidasSnpsError) as ei:
                abi.genes_curves(ctx, body, 50, S, S, orders, need, form=form, out=out)
            assert ei.value.status == abi.ERR_INVALID_ARG and ei.value.bad is None and all(w in ei.value.message for w in words), ei.value.message
            assert all((a == -7).all() for a in out)
    twice = good.copy()
    twice[2, 5] = twice[2, 1]
    refused(twice, need, ("row 2", "twice"))
    first = good.copy()
    first[0, 3] = first[0, 4]
    refused(first, need, ("row 0", "twice"))
    beyond = good.copy()
    beyond[1, 0] = S
    refused(beyond, need, ("row 1", "column %d" % S))
    negative = good.copy()
    negative[1, 7] = -1
    refused(negative, need, ("row 1",))
    other = good.copy()
    other[2, list(other[2]).index(3)] = 9                  # a column in use by the matrix, not by row 0
    refused(other, need, ("row 2", "row 0"))
    low, high = need.copy(), need.copy()
    low[4], high[6] = 0, 7
    refused(good, low, ("need", "row 4"))
    refused(good, high, ("need", "row 6"))
    out = [np.full(good.shape, -7, np.int64) for _ in range(3)]
    got = abi.genes_curves(ctx, body, 50, S, S, good, need, out=out)
    _same(got, _expect(present, good, need.tolist()), 'good orders')
    assert got['pan'] is out[0] and (out[0] >= 0).all()


def test_a_malformed_cell_is_reported_where_compare_genes_reports_it(ctx):
    S = 6
    rows = [r.split(b'\t') for r in _body(_case(S, 150, seed=4)).tobytes().split(b'\n')[:-1]]
    rows[100][2] = b'NA'
    rows[80].append(b'1.0')
    rows[50][5] = b'inf'
    rows[50][3] = b''
    body = np.frombuffer(b'\n'.join(b'\t'.join(r) for r in rows) + b'\n', np.uint8)
    need = genes_curves.need_table(S, 0.9)
    orders = _orders(range(S), 3, seed=2)
    out = [np.full(orders.shape, -7, np.int64) for _ in range(3)]
    for group_rows, chunk in ((0, 0), (40, 0), (7, 2048), (49, 0), (50, 0)):
        with pytest.raises(abi.MidasSnpsError) as ec:
            ctx.genes_compare(body, len(rows), S, S, group_rows=group_rows, chunk_bytes=chunk)
        for form in (0, 1):
            with pytest.raises(abi.MidasSnpsError) as ei:
                abi.genes_curves(ctx, body, len(rows), S, S, orders, need, form=form, group_rows=group_rows, chunk_bytes=chunk, out=out)
            assert ei.value.status == ec.value.status == abi.ERR_BAD_LAYOUT and ei.value.bad == ec.value.bad == (2, 50, 2), (group_rows, ei.value.bad)
    assert all((a == -7).all() for a in out)
    with pytest.raises(abi.MidasSnpsError) as ei:
        abi.genes_curves(ctx, body, len(rows), 2, S, _orders(range(2), 2, seed=1), genes_curves.need_table(2, 0.9), group_rows=64)
    assert ei.value.bad == (1, 80, -1)
    assert abi.genes_curves(ctx, body, 50, S, S, orders, need, group_rows=32)['n_rows'] == 50


WALKS = CG.walker_cases()


@pytest.mark.parametrize("k", range(len(WALKS)), ids=[w[0] for w in WALKS])
def test_the_walk_of_the_rows_at_its_borders(ctx, k):
    name, body, n_rows, group_rows, chunk = WALKS[k]
    need = M.need_linear(6, 0.6)
    orders = _orders(range(6), 4, seed=k)
    cells, _ = CG.read_cells(body, n_rows, 6, 6)
    exp = M.curves(cells, 0.35, orders, need)
    _not_trivial(exp)
    for form in (0, 1):
        got = abi.genes_curves(ctx, body, n_rows, 6, 6, orders, np.array(need, np.int32), form=form, group_rows=group_rows, chunk_bytes=chunk)
        assert (got['n_rows'], got['groups'], got['group_rows'], got['chunk_bytes']) == CG.walk(body, n_rows, group_rows, chunk), name
        _same(got, exp, (name, form))


@pytest.mark.parametrize("group_rows,chunk", [(10, 0), (1, 0), (0, 0), (10, 64)])
def test_a_short_row_in_one_group_wins_over_a_bad_cell_in_the_next(ctx, group_rows, chunk):
    body, bad = CG.walker_bad_body()
    with pytest.raises(abi.MidasSnpsError) as ei:
        abi.genes_curves(ctx, body, 30, 6, 6, _orders(range(6), 2, seed=1), genes_curves.need_table(6, 0.9), group_rows=group_rows, chunk_bytes=chunk)
    assert ei.value.status == abi.ERR_BAD_LAYOUT and ei.value.bad == bad


def test_two_calls_on_one_context_and_the_two_forms_give_equal_arrays(ctx):
    S = 90
    present = _mix(3000, S, seed=9)
    body = _text(present, seed=9)
    used = [s for s in range(S) if s % 7 != 3]
    orders = _orders(used, 9, seed=9)
    need = genes_curves.need_table(len(used), 0.8)
    exp = _expect(present, orders, need.tolist())
    _not_trivial(exp)
    calls = [abi.genes_curves(ctx, body, 3000, S, S, orders, need, form=form) for form in (1, 1, 0, 0)]
    for got in calls:
        _same(got, exp, 'twice')
    assert calls[0]['planes'] == 7 and calls[2]['planes'] == 0
    other = abi.genes_curves(ctx, body, 3000, S, S, _orders(used, 9, seed=10), need)
    assert np.array_equal(other['pan'][0], exp['pan'][0]) and not np.array_equal(other['pan'][1:], exp['pan'][1:])


def test_the_script_in_its_own_process_writes_the_models_tables_byte_for_byte(tmp_path):
    d = str(tmp_path / 'species_1')
    info = synth.write_pangenome_curve_dir(d, 700, 90, seed=11)
    text = open(os.path.join(d, 'genes_copynum.txt')).read()
    ids = str(tmp_path / 'ids.txt')
    lines = ['# every sample but each fifth'] + [id for k, id in enumerate(info['sample_ids'][:70]) if k % 5 != 2] + ['', info['sample_ids'][0]]
    with open(ids, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    out, orders_path = str(tmp_path / 'curves.txt'), str(tmp_path / 'orders.txt')
    for options, sample_lines, argv in (
            (dict(), None, []),
            (dict(core_frac=0.95, permutations=7, seed=3, cutoff=0.5, max_genes=650, max_samples=70), lines,
             ['--core_frac', '0.95', '--permutations', '7', '--seed', '3', '--samples', ids, '--cutoff', '0.5', '--max_genes', '650',
              '--max_samples', '70', '--group_rows', '77', '--chunk_bytes', '30000'])):
        table, orders, res = M.model_tables(text, options, sample_lines)
        _not_trivial(res)
        r = subprocess.run([sys.executable, SCRIPT, d, '--out', out, '--orders', orders_path] + argv, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        assert open(out).read() == table and open(orders_path).read() == orders
        for line in res['lines']:
            assert line in r.stdout.split('\n'), (line, r.stdout)
    assert res['pan'].shape == (8, 56) and "Samples in use: 56 of 70" in res['lines']
    with open(ids, 'a') as f:
        f.write('sample_777\n')
    r = subprocess.run([sys.executable, SCRIPT, d, '--out', out, '--samples', ids], capture_output=True, text=True, timeout=600)
    assert r.returncode == 1 and "Error: %s, line %d: the sample sample_777 is not among the 90 sample columns in use" % (ids, len(lines) + 1) in r.stderr


def test_merge_midas_genes_then_gene_curves_chain(tmp_path):
    from midas_amd import synth as reads_synth
    ds = reads_synth.make_pangenome_dataset(n_species=2, genes_per_species=60, n_reads=12000, seed=31)
    db = str(tmp_path / 'db')
    fq = str(tmp_path / 'reads.fq')
    with open(fq, 'w') as h:
        h.write("@r1\nACGT\n+\nIIII\n")
    rng = np.random.default_rng(3)
    dirs = []
    for k in range(4):
        idx = np.sort(rng.choice(ds['refid'].size, ds['refid'].size * (k + 2) // 6, replace=False))
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
        options = dict(core_frac=0.75, permutations=5, seed=2, cutoff=0.9)
        table, orders, res = M.model_tables(text, options)
        r = subprocess.run([sys.executable, SCRIPT, os.path.join(out, sp), '--out', str(tmp_path / 'c.txt'), '--orders', str(tmp_path / 'o.txt'),
                            '--core_frac', '0.75', '--permutations', '5', '--seed', '2', '--cutoff', '0.9'],
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        assert open(str(tmp_path / 'c.txt')).read() == table and open(str(tmp_path / 'o.txt')).read() == orders, sp
        assert res['pan'].shape == (6, 4) and res['pan'][0, 3] > 10
