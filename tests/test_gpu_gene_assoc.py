"""gene_assoc.py on the GPU box: midas_genes_assoc against the sequential model (tests/gene_assoc_model.py), every output array
equal with its dtype and every product equal cell for cell -- at used-sample counts around the MFMA's K step and the 64-sample
word with unused columns between the used ones, at kept-gene counts around the 16-row tile and the 32-row workgroup with
dropped genes between kept ones, at relabelling counts around the 16-column tile, at three group settings and with both forms
of the product; the operand map on an identity matrix; the border between the two 7-bit digits; ties; the limits; a malformed
cell; the script and the chain merge_midas.py genes -> gene_assoc.py.

One deviation from the letter of the issue: a doubled midrank of 127 needs a tie of two (2 * 62 + 2 + 1) and 128 a value of its
own above 63 others, so the two cannot stand in one row; the digit border is held by a row whose cases hold 127 and 127 and a
row whose cases hold 126 and 128."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from midas_amd import abi
from midas_amd.analyze import genes_assoc, synth
from tests import compare_genes_model as CG
from tests import gene_assoc_model as M
from tests.test_gpu_compare_genes import _write_gene_info

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPT = os.path.join(ROOT, 'scripts', 'gene_assoc.py')
GROUPS = ((0, 0), (100, 4096), (77, 1500))      # the three settings of test_gpu_gene_linkage.py
ARRAYS = (('row_of_slot', np.int32), ('count', np.int32), ('count_case', np.int32), ('w', np.int64), ('ties', np.int64), ('exceed', np.uint32),
          ('products', np.int32))
PRESENT, ABSENT = ('1.5', '0.36', '0.3500001', '7e-1', '12', '2.25', '1.5'), ('0.0', '0.35', '0.21', '0', '3.4e-1', '0.0', '-0.0')
NS = (2, 7, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200)
KS = (1, 15, 16, 17, 31, 32, 33, 100)
PS = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 200)


def _triples():
    """Every value of each axis with at least two values of the others; every second one ends in an unused column."""
    t = []
    for i, N in enumerate(NS):
        t += [(N, KS[i % 8], PS[i % 11]), (N, KS[(i + 3) % 8], PS[(i + 5) % 11])]
    for i, K in enumerate(KS):
        t += [(NS[(2 * i + 1) % 12], K, PS[(3 * i) % 11]), (NS[(5 * i + 2) % 12], K, PS[(3 * i + 4) % 11])]
    for i, P in enumerate(PS):
        t += [(NS[(5 * i) % 12], KS[(i + 1) % 8], P), (NS[(7 * i + 3) % 12], KS[(3 * i + 2) % 8], P)]
    t = sorted(set(t))
    for axis, values in enumerate((NS, KS, PS)):
        for v in values:
            for other in {0, 1, 2} - {axis}:
                assert len({x[other] for x in t if x[axis] == v}) >= 2, (axis, v)
    return t


TRIPLES = _triples()


@pytest.fixture(scope="module")
def ctx():
    with abi.Context(0) as c:
        yield c


def _columns(N, seed, unused_last):
    """-> (S, used columns, case columns): unused columns stand between the used ones; the last column is used or not."""
    rng = np.random.default_rng(seed)
    gaps = rng.integers(0, 3, N)                        # unused columns in front of every used one
    used = (np.cumsum(gaps + 1) - 1).tolist()
    S = used[-1] + 1 + (1 + int(rng.integers(0, 3)) if unused_last else 0)
    n1 = max(1, min(N - 1, N // 3)) if N > 1 else 1
    case = sorted(rng.permutation(used)[:n1].tolist())
    return S, used, case


def _limits(N):
    return (2, 2) if N >= 5 else (1, 1)


def _body(N, K, seed, S, used):
    """Rows with exactly K kept genes under _limits(N) and dropped genes between them.  The first kept row stands exactly on
    min_present, the second on min_absent; the dropped rows stand one off either border.  The used cells hold few distinct
    values (many ties) in several spellings; the unused columns hold anything, mostly present."""
    rng = np.random.default_rng(seed)
    lo, ab = _limits(N)
    rows = []
    for k in range(K):
        c = lo if k == 0 else N - ab if k == 1 else int(rng.integers(lo, N - ab + 1))
        counts = [c] + [(lo - 1, N - ab + 1)[(k + j) % 2] for j in range(int(rng.integers(0, 3)))]
        for c in counts:
            present = np.zeros(N, bool)
            present[rng.permutation(N)[:c]] = True
            few = int(rng.integers(1, 8))
            cells = [PRESENT[int(rng.integers(0, 7))] for _ in range(S)]
            for j, col in enumerate(used):
                cells[col] = (PRESENT if present[j] else ABSENT)[int(rng.integers(0, few))]
            rows.append('g%d\t%s' % (len(rows), '\t'.join(cells)))
    return np.frombuffer(('\n'.join(rows) + '\n').encode(), np.uint8)


def _same(got, exp, what):
    for k, dt in ARRAYS:
        assert got[k].dtype == dt and got[k].shape == exp[k].shape and np.array_equal(got[k], exp[k]), (what, k)
    for k in ('n_rows', 'n_used', 'n_case', 'n_kept', 'n_perms'):
        assert got[k] == exp[k], (what, k)


def _run(ctx, body, S, used, case, planes, dtype, what, groups=GROUPS, forms=(0, 1), n_rows=None, **kw):
    n = int((body == 10).sum()) if n_rows is None else n_rows
    cells, _ = CG.read_cells(body, n, S, S)
    exp = M.stats(cells, used, case, planes, kw.get('cutoff', 0.35), dtype, kw.get('min_present', 1), kw.get('min_absent', 0))
    use, cs = genes_assoc.words_of(used, S), genes_assoc.words_of(case, S)
    seen = []
    for group_rows, chunk in groups:
        for form in forms:
            got = ctx.genes_assoc(body, n, S, S, use, cs, planes, dtype=dtype, group_rows=group_rows, chunk_bytes=chunk, form=form, products=True, **kw)
            _same(got, exp, (what, dtype, group_rows, chunk, form))
            assert got['form'] == form
            seen.append(got)
    return exp, seen


@pytest.mark.parametrize("N,K,P", TRIPLES)
def test_the_device_equals_the_model_around_the_k_step_the_tiles_and_the_word(ctx, N, K, P):
    unused_last = (N + K + P) % 2 == 1
    S, used, case = _columns(N, seed=N * 1000 + K, unused_last=unused_last)
    assert len(used) == N and (used[-1] == S - 1) != unused_last
    lo, ab = _limits(N)
    body = _body(N, K, seed=P * 1000 + K, S=S, used=used)
    planes = genes_assoc.permutation_planes(used, len(case), P, seed=N + P, n_samples=S)
    for dtype in ('presabs', 'copynum'):
        exp, seen = _run(ctx, body, S, used, case, planes, dtype, (N, K, P), min_present=lo, min_absent=ab)
        assert exp['n_kept'] == K and (exp['n_rows'] > K or K == 1)
        c = exp['count']
        assert c[0] == lo and (K < 2 or c[1] == N - ab)
        assert seen[0]['groups'] == 1 and (exp['n_rows'] <= 100 or seen[2]['groups'] > 1) and seen[1]['in_lds'] == 1
    assert N < 7 or exp['ties'].max() > 0


def test_the_operand_map_on_an_identity_matrix(ctx):
    """presabs, gene g present in used sample g alone: the product of gene g and relabelling b is bit g of plane b, so a row or a
    column of either MFMA operand in another lane's place shows as a wrong cell."""
    N = 70
    S, used, case = _columns(N, seed=5, unused_last=True)
    rng = np.random.default_rng(9)
    rows = []
    for g in range(N):
        cells = [PRESENT[int(rng.integers(0, 7))] for _ in range(S)]
        for j, col in enumerate(used):
            cells[col] = '1.5' if j == g else '0.0'
        rows.append('g%d\t%s' % (g, '\t'.join(cells)))
    body = np.frombuffer(('\n'.join(rows) + '\n').encode(), np.uint8)
    P = 37
    planes = genes_assoc.permutation_planes(used, len(case), P, seed=3, n_samples=S)
    exp, seen = _run(ctx, body, S, used, case, planes, 'presabs', 'identity')
    bit = np.array([[(int(planes[b, c >> 6]) >> (c & 63)) & 1 for b in range(P)] for c in used], np.int32)
    assert len({row.tobytes() for row in bit}) > 60 and len({col.tobytes() for col in bit.T}) == P          # asymmetric
    for got in seen:
        assert np.array_equal(got['products'], bit)
    assert len(set(exp['exceed'].tolist())) > 1 and exp['n_kept'] == N


def _distinct_row(N, S, used, order, name='d'):
    """A row whose used sample used[order[k]] holds the k-th smallest of N distinct values."""
    cells = ['0.25'] * S
    for k, j in enumerate(order):
        cells[used[j]] = '%d.5' % k
    return '%s\t%s' % (name, '\t'.join(cells))


def test_the_border_between_the_two_digits(ctx):
    """N = 63: every doubled midrank is below 128, the high digit is 0 throughout; N = 65: the top rank is 130.  Then rows of 70
    samples whose case samples hold 127 twice (a tie of two above 62 others), and 126 and 128."""
    for N in (63, 65):
        S, used, case = _columns(N, seed=N, unused_last=False)
        order = np.random.default_rng(N).permutation(N).tolist()
        body = np.frombuffer((_distinct_row(N, S, used, order) + '\n').encode(), np.uint8)
        planes = genes_assoc.permutation_planes(used, len(case), 33, seed=N, n_samples=S)
        exp, _ = _run(ctx, body, S, used, case, planes, 'copynum', ('distinct', N))
        assert exp['ties'].tolist() == [0] and exp['products'].max() <= sum(range(2 * N, 2 * (N - len(case)), -2))
    N = 70
    S, used, _ = _columns(N, seed=70, unused_last=True)
    order = list(range(N))
    tied = _distinct_row(N, S, used, order, 'tied').split('\t')
    tied[1 + used[63]] = tied[1 + used[62]]                        # samples 62 and 63: 62 below, a tie of two: 2 * 62 + 2 + 1 = 127
    body = np.frombuffer(('\t'.join(tied) + '\n' + _distinct_row(N, S, used, order, 'apart') + '\n').encode(), np.uint8)
    planes = genes_assoc.permutation_planes(used, 2, 65, seed=1, n_samples=S)
    exp, _ = _run(ctx, body, S, used, [used[62], used[63]], planes, 'copynum', '127 and 127; 126 and 128')
    assert exp['w'].tolist() == [127 + 127, 126 + 128] and exp['ties'].tolist() == [6, 0]


def test_ties(ctx):
    N = 40
    S, used, case = _columns(N, seed=40, unused_last=True)
    a, b = '1.0', '1.0000000000000002'
    assert CG.pandas_float(b)[0] == math.nextafter(CG.pandas_float(a)[0], 2.0)          # one ulp apart after pandas' conversion

    def row(name, fill):
        cells = ['3.5'] * S
        for j, col in enumerate(used):
            cells[col] = fill(j)
        return '%s\t%s' % (name, '\t'.join(cells))
    rows = [row('one_cell', lambda j: '2.5' if j == 17 else '0.0'),
            row('two_groups', lambda j: '0.5' if j % 3 else '1.5'),
            row('all_equal', lambda j: '0.75'),
            row('signed_zero', lambda j: ('-0.0', '0.0', '0', '-0')[j % 4] if j != 5 else '1.0'),
            row('one_ulp', lambda j: a if j % 2 else b)]
    body = np.frombuffer(('\n'.join(rows) + '\n').encode(), np.uint8)
    P = 50
    planes = genes_assoc.permutation_planes(used, len(case), P, seed=2, n_samples=S)
    exp, _ = _run(ctx, body, S, used, case, planes, 'copynum', 'ties', cutoff=-1.0)
    t = lambda *sizes: sum(n ** 3 - n for n in sizes)
    assert exp['ties'].tolist() == [t(39), t(14, 26), t(40), t(39), t(20, 20)]
    assert exp['exceed'][2] == P and (exp['products'][2] == len(case) * (N + 1)).all()
    _run(ctx, body, S, used, case, planes, 'presabs', 'ties', cutoff=0.6, forms=(1,))


def test_a_tile_whose_digits_do_not_fit_the_lds(ctx):
    """1 000 used samples: the two digits of 32 rows take 65 KB, so the A fragments come from memory; 33 kept rows: two tiles."""
    N, K, P = 1000, 33, 17
    S, used, case = _columns(N, seed=1000, unused_last=True)
    body = _body(N, K, seed=1000, S=S, used=used)
    planes = genes_assoc.permutation_planes(used, len(case), P, seed=4, n_samples=S)
    exp, seen = _run(ctx, body, S, used, case, planes, 'copynum', 'beyond the lds', groups=((0, 0), (20, 0)), min_present=2, min_absent=2)
    assert exp['n_kept'] == K and all(g['in_lds'] == 0 for g in seen) and exp['products'].max() > 127 * 128


def test_the_limits(ctx):
    N = 8191
    used = list(range(N))
    order = np.random.default_rng(8).permutation(N).tolist()
    case = sorted(order[-3:] + order[:40])                           # the sample with the greatest value is a case
    body = np.frombuffer((_distinct_row(N, N, used, order) + '\n').encode(), np.uint8)
    planes = genes_assoc.permutation_planes(used, len(case), 16, seed=8, n_samples=N)
    for dtype in ('presabs', 'copynum'):
        exp, seen = _run(ctx, body, N, used, case, planes, dtype, N, groups=((0, 0),))
        assert exp['n_kept'] == 1 and all(g['in_lds'] == 0 for g in seen)
    assert exp['w'][0] >= 16382 + 16380 + 16378 and exp['ties'][0] == 0
    # one sample more
    N = 8192
    wide = np.frombuffer(('g\t' + '\t'.join(['1.5'] * N) + '\n').encode(), np.uint8)
    use = genes_assoc.words_of(range(N), N)
    with pytest.raises(abi.MidasSnpsError) as ei:
        ctx.genes_assoc(wide, 1, N, N, use, genes_assoc.words_of(range(5), N), np.zeros((0, N // 64), np.uint64))
    assert ei.value.status == abi.ERR_UNSUPPORTED
    use[-1] = np.uint64(use[-1]) >> np.uint64(1)                     # 8 191 of the 8 192 columns: fine
    assert ctx.genes_assoc(wide, 1, N, N, use, genes_assoc.words_of(range(5), N), np.zeros((0, N // 64), np.uint64))['n_kept'] == 1
    # more than 2^24 products asked for; more than 1 000 000 relabellings
    rows = np.frombuffer(''.join('g%d\t1.5\t0.0\n' % r for r in range(1100)).encode(), np.uint8)
    rng = np.random.default_rng(1)
    planes = np.where(rng.random((16000, 1)) < 0.5, np.uint64(1), np.uint64(2))
    use, cs = genes_assoc.words_of([0, 1], 2), genes_assoc.words_of([0], 2)
    with pytest.raises(abi.MidasSnpsError) as ei:
        ctx.genes_assoc(rows, 1100, 2, 2, use, cs, planes, products=True)
    assert ei.value.status == abi.ERR_INVALID_ARG and 1100 * 16000 > 1 << 24
    got = ctx.genes_assoc(rows, 1100, 2, 2, use, cs, planes)
    assert got['n_kept'] == 1100 and (got['exceed'] == 16000).all()
    with pytest.raises(abi.MidasSnpsError) as ei:
        ctx.genes_assoc(rows, 10, 2, 2, use, cs, np.ones((1000001, 1), np.uint64))
    assert ei.value.status == abi.ERR_INVALID_ARG


def test_a_malformed_cell_is_reported_where_compare_genes_reports_it(ctx):
    S, used, case = 6, [0, 2, 3, 5], [0, 3]
    rows = [r.split(b'\t') for r in _body(4, 150, seed=4, S=S, used=used).tobytes().split(b'\n')[:-1]]
    rows[100][2] = b'NA'
    rows[80].append(b'1.0')
    rows[50][5] = b'inf'
    rows[50][3] = b''                                                # (column 4 is not a used one; column 2 is the row's first bad cell)
    body = np.frombuffer(b'\n'.join(b'\t'.join(r) for r in rows) + b'\n', np.uint8)
    use, cs = genes_assoc.words_of(used, S), genes_assoc.words_of(case, S)
    planes = genes_assoc.permutation_planes(used, 2, 8, 0, S)
    for group_rows, chunk in ((0, 0), (40, 0), (7, 2048), (49, 0), (50, 0)):
        with pytest.raises(abi.MidasSnpsError) as ec:
            ctx.genes_compare(body, len(rows), S, S, group_rows=group_rows, chunk_bytes=chunk)
        with pytest.raises(abi.MidasSnpsError) as ei:
            ctx.genes_assoc(body, len(rows), S, S, use, cs, planes, group_rows=group_rows, chunk_bytes=chunk)
        assert ei.value.status == ec.value.status == abi.ERR_BAD_LAYOUT and ei.value.bad == ec.value.bad == (2, 50, 2), (group_rows, ei.value.bad)
    with pytest.raises(abi.MidasSnpsError) as ei:
        ctx.genes_assoc(body, len(rows), 2, S, genes_assoc.words_of([0, 1], 2), genes_assoc.words_of([0], 2), np.zeros((0, 1), np.uint64), group_rows=64)
    assert ei.value.bad == (1, 80, -1)
    assert ctx.genes_assoc(body, 50, S, S, use, cs, planes, group_rows=32)['n_rows'] == 50


def _table(path):
    with open(path) as f:
        return f.read()


def test_the_script_in_its_own_process_writes_the_models_table_byte_for_byte(tmp_path):
    d = str(tmp_path / 'species_1')
    info = synth.write_assoc_genes_dir(d, 600, 90, seed=11, associated=0.05)
    text, groups = _table(os.path.join(d, 'genes_copynum.txt')), _table(info['groups_path'])
    out = str(tmp_path / 'assoc.txt')
    for options, argv in ((dict(), []),
                          (dict(dtype='copynum', permutations=300, seed=5), ['--dtype', 'copynum', '--permutations', '300', '--seed', '5']),
                          (dict(permutations=130, seed=2, min_present=5, min_absent=9, cutoff=0.5, max_samples=70, max_genes=550, case='control'),
                           ['--permutations', '130', '--seed', '2', '--min_present', '5', '--min_absent', '9', '--cutoff', '0.5', '--max_samples', '70',
                            '--max_genes', '550', '--case', 'control', '--group_rows', '77', '--chunk_bytes', '30000']),
                          (dict(dtype='copynum', permutations=40, seed=1), ['--dtype', 'copynum', '--permutations', '40', '--seed', '1', '--form', '0'])):
        table, res = M.model_tables(text, groups, options)
        r = subprocess.run([sys.executable, SCRIPT, d, '--groups', info['groups_path'], '--out', out] + argv, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        assert _table(out) == table
        assert res['n_kept'] > 100 and "Rows read: %d" % res['n_rows'] in r.stdout.split('\n') and "): %d\n" % res['n_kept'] in r.stdout
    # the planted genes are what the test finds
    table, res = M.model_tables(text, groups, dict(dtype='copynum', permutations=300, seed=5))
    q = np.array([float(line.split('\t')[5]) for line in table.split('\n')[1:-1]])
    planted = info['planted'][res['row_of_slot']]
    assert planted.sum() > 10 and (q[planted] < 0.05).mean() > 0.8 and (q[~planted] < 0.05).mean() < 0.05


def test_merge_midas_genes_then_gene_assoc_chain(tmp_path):
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
        text = _table(os.path.join(out, sp, 'genes_copynum.txt'))
        ids = text.split('\n')[0].split('\t')[1:]
        assert text.count('\n') > 10 and len(ids) == 4
        groups = str(tmp_path / 'groups.txt')
        with open(groups, 'w') as f:
            f.write('sample_id\tsite\n%s\tgut\n%s\toral\n%s\tgut\n' % (ids[0], ids[1], ids[3]))
        for dtype in ('presabs', 'copynum'):
            options = dict(dtype=dtype, permutations=24, seed=4, cutoff=0.9)
            table, res = M.model_tables(text, _table(groups), options)
            r = subprocess.run([sys.executable, SCRIPT, os.path.join(out, sp), '--groups', groups, '--out', str(tmp_path / 'a.txt'), '--dtype', dtype,
                                '--permutations', '24', '--seed', '4', '--cutoff', '0.9'], capture_output=True, text=True, timeout=600)
            assert r.returncode == 0, r.stderr
            assert _table(str(tmp_path / 'a.txt')) == table, (sp, dtype)
            assert res['n_kept'] > 10 and res['n_used'] == 3 and "left out: 1" in r.stdout
