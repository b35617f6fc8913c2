"""gene_linkage.py on the GPU box: midas_genes_linkage against the sequential model (tests/gene_linkage_model.py), every output
array equal and every integer exact -- at sample counts around the 64-sample word and just above each word count at which the
pair kernel changes form, at kept-gene counts around the 64-anchor strip and the 256-partner step, with dropped genes between
kept ones, at three group settings; the borders of need[]; a chain whose labels take several rounds; max_pairs; a malformed cell;
the script and the chain merge_midas.py genes -> gene_linkage.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

from midas_amd import abi
from midas_amd.analyze import genes_linkage, synth
from tests import compare_genes_model as CG
from tests import gene_linkage_model as M
from tests.test_gpu_compare_genes import _write_gene_info

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPT = os.path.join(ROOT, 'scripts', 'gene_linkage.py')
GROUPS = ((0, 0), (100, 4096), (77, 1500))      # one group; groups of 100 rows or a 4 KiB chunk's; 77 rows or a smaller chunk's
ARRAYS = ('count', 'row_of_slot', 'label', 'pair_a', 'pair_b', 'pair_both')
PRESENT, ABSENT = ('1.5', '0.36', '0.3500001', '7e-1', '12'), ('0.0', '0.35', '0.21', '0', '3.4e-1')


@pytest.fixture(scope="module")
def ctx():
    with abi.Context(0) as c:
        yield c


def _body(present, seed=0):
    """The rows after the header for a presence matrix [genes][samples]: present cells above the cutoff 0.35, absent ones at it
    or below, in several spellings."""
    rng = np.random.default_rng(seed)
    present = np.asarray(present, bool)
    pick = rng.integers(0, 5, present.shape)
    lines = ['g%d\t%s' % (g, '\t'.join((PRESENT if present[g, s] else ABSENT)[pick[g, s]] for s in range(present.shape[1])))
             for g in range(present.shape[0])]
    return np.frombuffer(('\n'.join(lines) + '\n').encode(), np.uint8)


def _case(S, K, seed):
    """A presence matrix with exactly K kept genes under min_present = min_absent = 2 and dropped genes between them: the last
    column is empty; the kept genes are copies of a few profiles with up to two cells flipped, their counts forced into
    [2, S - 2], the first two kept ones standing exactly at 2 and at S - 2; the dropped ones have 0, 1 or S - 1 cells set: one
    off each border, and none."""
    rng = np.random.default_rng(seed)
    pool = rng.random((max(2, K // 6 + 1), S)) < rng.uniform(0.3, 0.7, (max(2, K // 6 + 1), 1))
    rows = []
    for k in range(K):
        p = pool[rng.integers(0, pool.shape[0])].copy()
        p[rng.integers(0, S, rng.integers(0, 3))] ^= True
        if k == 0:
            p[:] = False
            p[:2] = True                                   # c = min_present
        elif k == 1 and S >= 5:
            p[:] = True
            p[S - 2:] = False                              # S - c = min_absent
        p[S - 1] = False
        order = rng.permutation(S - 1)
        for s in order:                                    # into [2, S - 2]
            if p.sum() >= 2:
                break
            p[s] = True
        for s in order:
            if S - p.sum() >= 2:
                break
            p[s] = False
        rows.append(p)
        for c in ((0, 1, S - 1)[(k + j) % 3] for j in range(int(rng.integers(0, 3)))):      # dropped genes behind it
            d = np.zeros(S, bool)
            d[:c] = True
            rows.append(d)
    return np.array(rows, bool)


def _expect(body, S, need, min_present=2, min_absent=2, cutoff=0.35, n_rows=None):
    n = int((body == 10).sum()) if n_rows is None else n_rows
    cells, _ = CG.read_cells(body, n, S, S)
    return M.link(cells, cutoff, min_present, min_absent, need)


def _same(got, exp, what):
    for k in ARRAYS:
        assert got[k].dtype == np.int32 and np.array_equal(got[k], exp[k]), (what, k)
    assert got['n_kept'] == exp['n_kept'] and got['visited'] == exp['visited'] and got['linked'] == exp['linked'], what


def _run(ctx, body, S, need, what, exp=None, forms=(0,), **kw):
    n = int((body == 10).sum())
    exp = exp if exp is not None else _expect(body, S, need, kw.get('min_present', 2), kw.get('min_absent', 2))
    seen = []
    for group_rows, chunk in GROUPS:
        for form in forms:
            got = ctx.genes_linkage(body, n, S, S, np.array(need, np.int32), group_rows=group_rows, chunk_bytes=chunk, pair_form=form, **kw)
            assert got['n_rows'] == n
            _same(got, exp, (what, group_rows, chunk, form))
            seen.append(got)
    return exp, seen


@pytest.mark.parametrize("S", [7, 64, 65, 130])
@pytest.mark.parametrize("K", [1, 63, 64, 65, 129, 257, 300])
def test_the_device_equals_the_model_around_the_word_the_strip_and_the_step(ctx, S, K):
    present = _case(S, K, seed=1000 * S + K)
    assert not present[:, S - 1].any()
    body = _body(present, seed=K)
    need = M.need_linear(S, 0.6)
    assert genes_linkage.need_table(S, 0.6).tolist() == need
    exp, seen = _run(ctx, body, S, need, (S, K), forms=(0, 1))
    assert exp['n_kept'] == K and present.shape[0] > K or K == 1
    assert K < 3 or 0 < exp['linked'] < exp['visited']
    c = exp['count']
    assert K < 2 or S < 5 or (c[0] == 2 and c[1] == S - 2)
    assert seen[0]['groups'] == 1 and (present.shape[0] <= 100 or seen[2]['groups'] > 1)
    assert seen[0]['strips'] == (K + 63) // 64 and seen[0]['form'] == (1 if S <= 64 else 2 if S <= 128 else 4) and seen[1]['form'] == 0


@pytest.mark.parametrize("S,form,K", [(129, 4, 40), (257, 8, 40), (513, 16, 40), (1025, 0, 40), (4100, 0, 16)])
def test_one_sample_count_just_above_each_word_count_at_which_the_pair_kernel_changes_form(ctx, S, form, K):
    """3, 5, 9 and 17 words: the first widths kept in 4, 8 and 16 registers and the first read word by word; 4100 samples:
    need[] no longer lies in LDS."""
    present = _case(S, K, seed=S)
    present[:, [0, S - 1]] = present[:, [S - 1, 0]]      # the empty column first: the lone sample of the last word is in use
    body = _body(present, seed=S)
    need = M.need_linear(S, 0.9)
    exp, seen = _run(ctx, body, S, need, S)
    assert exp['n_kept'] == K and 0 < exp['linked'] < exp['visited'] and all(g['form'] == form for g in seen)
    assert present[:, (S - 1) // 64 * 64:].any()          # the last word holds set bits, and pad bits unless S is a multiple of 64


def test_a_pair_exactly_at_need_and_one_below_it(ctx):
    S, T = 20, 0.75
    need = M.need_linear(S, T)
    assert need[8] == 6 and need[9] == 7

    def gene(*samples):
        p = np.zeros(S, bool)
        p[list(samples)] = True
        return p
    rows = [gene(0, 1, 2, 3, 4, 5, 6, 7),        # a
            gene(0, 1, 2, 3, 4, 5),              # both 6 of either 8: at need[8]
            gene(0, 1, 2, 3, 4),                 # both 5 of either 8: one below
            gene(0, 1, 2, 3, 4, 5, 8),           # both 6 of either 9: need[9] is 7
            gene(0, 1, 2, 3, 4, 5, 6, 8)]        # both 7 of either 9: at need[9]
    exp, _ = _run(ctx, _body(np.array(rows)), S, need, 'borders')
    linked_to_a = [(a, b, c) for a, b, c in zip(exp['pair_a'].tolist(), exp['pair_b'].tolist(), exp['pair_both'].tolist()) if a == 0]
    assert linked_to_a == [(0, 1, 6), (0, 4, 7)]


def test_a_threshold_of_one_links_identical_profiles_only(ctx):
    S = 70
    present = _case(S, 90, seed=5)
    present = np.concatenate([present, present[::3]])
    need = genes_linkage.need_table(S, 1.0).tolist()
    exp, _ = _run(ctx, _body(present, seed=2), S, need, 'T = 1')
    assert exp['linked'] >= 30
    c = exp['count']
    assert np.array_equal(c[exp['pair_a']], exp['pair_both']) and np.array_equal(c[exp['pair_b']], exp['pair_both'])


def test_steps_without_a_pair_between_steps_with_one(ctx):
    """800 kept genes with profiles of their own, T = 1.0: strip 0 meets a pair in its steps 0 and 2 and none in step 1, strip 1
    none before its step 2 -- the write pass skips the steps the count pass found empty and still lands every pair."""
    S = 70
    rng = np.random.default_rng(12)
    present = rng.random((800, S)) < 0.5
    present[5] = present[3]
    present[700] = present[3]
    present[650] = present[100]
    assert len({row.tobytes() for row in present}) == 797 and present.sum(axis=1).min() >= 2 and present.sum(axis=1).max() <= S - 2
    exp, seen = _run(ctx, _body(present, seed=1), S, genes_linkage.need_table(S, 1.0).tolist(), 'empty steps', forms=(0, 1))
    assert list(zip(exp['pair_a'].tolist(), exp['pair_b'].tolist())) == [(3, 5), (3, 700), (5, 700), (100, 650)]
    assert exp['label'][700] == 3 and exp['label'][650] == 100 and seen[0]['strips'] == 13


def test_count_borders_of_min_present_and_min_absent(ctx):
    S = 12
    rows = np.zeros((8, S), bool)
    for g, c in enumerate((2, 3, 4, 5, 8, 9, 10, 11)):
        rows[g, :c] = True
    need = M.need_linear(S, 0.5)
    for min_present, min_absent, kept in ((3, 3, [3, 4, 5, 8, 9]), (4, 2, [4, 5, 8, 9, 10]), (1, 0, [2, 3, 4, 5, 8, 9, 10, 11]), (9, 1, [9, 10, 11]),
                                          (13, 0, []), (1, 13, [])):
        exp, _ = _run(ctx, _body(rows), S, need, (min_present, min_absent), min_present=min_present, min_absent=min_absent)
        assert exp['count'].tolist() == kept


def test_a_chain_of_120_genes_takes_more_than_one_round_of_labels(ctx):
    """Gene i is present in samples i .. i + 9 of 130; at T = 0.8 neighbours (9 of 11) are linked and next-but-one genes (8 of
    12) are not.  The rows are written last gene first, so the slots descend along the chain."""
    S, n = 130, 120
    present = np.zeros((n, S), bool)
    for r in range(n):
        i = n - 1 - r
        present[r, i:i + 10] = True
    need = M.need_linear(S, 0.8)
    assert need[11] == 9 and need[12] == 10
    exp, seen = _run(ctx, _body(present), S, need, 'chain')
    assert exp['linked'] == n - 1 and np.array_equal(exp['pair_b'], exp['pair_a'] + 1) and not exp['label'].any()
    assert all(g['label_rounds'] > 1 for g in seen)


def test_two_components_a_singleton_and_min_group(ctx, tmp_path):
    S = 16
    profile = lambda *s: [k in s for k in range(S)]
    rows = [profile(0, 1, 2, 3), profile(8, 9, 10), profile(0, 1, 2, 3), profile(5, 6), profile(8, 9, 10), profile(0, 1, 2, 3), profile(12, 13),
            profile(0, 1, 2, 3, 4)]
    text = M.matrix_text(['gene_%d' % g for g in range(len(rows))], ['s%d' % s for s in range(S)], rows)
    d = CG.write_dir(str(tmp_path / 'species_1'), text)
    m = abi.GenesMatrix(os.path.join(d, 'genes_copynum.txt'))
    need = genes_linkage.need_table(S, 0.8)
    got = ctx.genes_linkage(m.text, m.n_rows, S, S, need)
    assert got['label'].tolist() == [0, 1, 0, 3, 1, 0, 6, 0] and got['linked'] == 7
    for min_group, n_groups in ((2, 2), (3, 1), (5, 0)):
        assert m.write_groups(str(tmp_path / 'g.txt'), got, min_group) == n_groups
        assert open(str(tmp_path / 'g.txt')).read() == M.groups_text(['gene_%d' % g for g in range(len(rows))], got, min_group)[0]
    m.write_linkage(str(tmp_path / 'p.txt'), got)
    assert open(str(tmp_path / 'p.txt')).read() == M.model_tables(text, dict(min_jaccard=0.8))[0]
    r = subprocess.run([sys.executable, SCRIPT, d, '--out', str(tmp_path / 'p2.txt'), '--groups', str(tmp_path / 'g2.txt'), '--min_jaccard', '0.8',
                        '--min_group', '3'], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert open(str(tmp_path / 'g2.txt')).read() == M.model_tables(text, dict(min_jaccard=0.8, min_group=3))[1]
    assert "Groups of at least 3 genes: 1" in r.stdout


def test_max_pairs_one_below_the_total_is_an_error_that_writes_nothing(ctx):
    S = 65
    body = _body(_case(S, 130, seed=9), seed=9)
    need = M.need_linear(S, 0.6)
    exp = _expect(body, S, need)
    total, n = exp['linked'], int((body == 10).sum())
    assert total > 100
    out = [np.full(total + 64, -7, np.int32) for _ in range(3)]
    for group_rows, chunk in GROUPS:
        with pytest.raises(abi.MidasSnpsError) as ei:
            ctx.genes_linkage(body, n, S, S, np.array(need, np.int32), max_pairs=total - 1, group_rows=group_rows, chunk_bytes=chunk, pair_out=out)
        assert ei.value.status == abi.ERR_OUT_OF_MEMORY and ei.value.linked == total and ei.value.bad is None
        assert all((a == -7).all() for a in out)
    got = ctx.genes_linkage(body, n, S, S, np.array(need, np.int32), max_pairs=total, pair_out=out)
    _same(got, exp, 'max_pairs == total')
    assert all((a[total:] == -7).all() for a in out) and np.array_equal(out[0][:total], exp['pair_a'])


def test_a_malformed_cell_is_reported_where_compare_genes_reports_it(ctx):
    S = 6
    rows = [r.split(b'\t') for r in _body(_case(S, 150, seed=4)).tobytes().split(b'\n')[:-1]]
    rows[100][2] = b'NA'
    rows[80].append(b'1.0')
    rows[50][5] = b'inf'
    rows[50][3] = b''
    body = np.frombuffer(b'\n'.join(b'\t'.join(r) for r in rows) + b'\n', np.uint8)
    need = genes_linkage.need_table(S, 0.9)
    for group_rows, chunk in ((0, 0), (40, 0), (7, 2048), (49, 0), (50, 0)):
        with pytest.raises(abi.MidasSnpsError) as ec:
            ctx.genes_compare(body, len(rows), S, S, group_rows=group_rows, chunk_bytes=chunk)
        with pytest.raises(abi.MidasSnpsError) as ei:
            ctx.genes_linkage(body, len(rows), S, S, need, group_rows=group_rows, chunk_bytes=chunk)
        assert ei.value.status == ec.value.status == abi.ERR_BAD_LAYOUT and ei.value.bad == ec.value.bad == (2, 50, 2), (group_rows, ei.value.bad)
    with pytest.raises(abi.MidasSnpsError) as ei:
        ctx.genes_linkage(body, len(rows), 2, S, genes_linkage.need_table(2, 0.9), group_rows=64)
    assert ei.value.bad == (1, 80, -1)
    assert ctx.genes_linkage(body, 50, S, S, need, group_rows=32)['n_rows'] == 50


WALKS = CG.walker_cases()


@pytest.mark.parametrize("k", range(len(WALKS)), ids=[w[0] for w in WALKS])
def test_the_walk_of_the_rows_at_its_borders(ctx, k):
    name, body, n_rows, group_rows, chunk = WALKS[k]
    need = M.need_linear(6, 0.6)
    exp = _expect(body, 6, need, n_rows=n_rows)
    assert exp['n_kept'] > 10 and 0 < exp['linked'] < exp['visited']
    got = ctx.genes_linkage(body, n_rows, 6, 6, np.array(need, np.int32), group_rows=group_rows, chunk_bytes=chunk)
    assert (got['n_rows'], got['groups'], got['group_rows'], got['chunk_bytes']) == CG.walk(body, n_rows, group_rows, chunk), name
    _same(got, exp, name)


@pytest.mark.parametrize("group_rows,chunk", [(10, 0), (1, 0), (0, 0), (10, 64)])
def test_a_short_row_in_one_group_wins_over_a_bad_cell_in_the_next(ctx, group_rows, chunk):
    body, bad = CG.walker_bad_body()
    with pytest.raises(abi.MidasSnpsError) as ei:
        ctx.genes_linkage(body, 30, 6, 6, genes_linkage.need_table(6, 0.9), group_rows=group_rows, chunk_bytes=chunk)
    assert ei.value.status == abi.ERR_BAD_LAYOUT and ei.value.bad == bad


def test_the_script_in_its_own_process_writes_the_models_tables_byte_for_byte(tmp_path):
    d = str(tmp_path / 'species_1')
    synth.write_linked_genes_dir(d, 700, 90, seed=11, groups=[5, 12, 30, 50])
    text = open(os.path.join(d, 'genes_copynum.txt')).read()
    for options, argv in ((dict(), []),
                          (dict(min_jaccard=0.75, min_group=6, min_present=5, min_absent=9, cutoff=0.5, max_samples=70, max_genes=650),
                           ['--min_jaccard', '0.75', '--min_group', '6', '--min_present', '5', '--min_absent', '9', '--cutoff', '0.5',
                            '--max_samples', '70', '--max_genes', '650', '--group_rows', '77', '--chunk_bytes', '30000'])):
        pairs, groups, res = M.model_tables(text, options)
        out, grp = str(tmp_path / 'pairs.txt'), str(tmp_path / 'groups.txt')
        r = subprocess.run([sys.executable, SCRIPT, d, '--out', out, '--groups', grp] + argv, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        assert open(out).read() == pairs and open(grp).read() == groups
        assert res['linked'] > 100 and groups.count('\n') > 20
        for line in ("Rows read: %d" % res['n_rows'], "Pairs of genes visited: %d" % res['visited']):
            assert line in r.stdout.split('\n')
        assert "): %d\n" % res['n_kept'] in r.stdout and "): %d\n" % res['linked'] in r.stdout
    r = subprocess.run([sys.executable, SCRIPT, d, '--out', out, '--max_pairs', '10'], capture_output=True, text=True, timeout=600)
    total = M.model_tables(text, dict())[2]['linked']
    assert r.returncode == 1 and "%d pairs of genes are linked, more than --max_pairs 10: raise --min_jaccard or --max_pairs" % total in r.stderr


def test_merge_midas_genes_then_gene_linkage_chain(tmp_path):
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
        options = dict(min_jaccard=0.6, min_present=1, min_absent=0, cutoff=0.9)
        pairs, groups, res = M.model_tables(text, options)
        r = subprocess.run([sys.executable, SCRIPT, os.path.join(out, sp), '--out', str(tmp_path / 'p.txt'), '--groups', str(tmp_path / 'g.txt'),
                            '--min_jaccard', '0.6', '--min_present', '1', '--min_absent', '0', '--cutoff', '0.9'],
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        assert open(str(tmp_path / 'p.txt')).read() == pairs and open(str(tmp_path / 'g.txt')).read() == groups, sp
        assert res['n_kept'] > 10
