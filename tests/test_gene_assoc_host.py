"""gene_assoc.py without a device: a case worked by hand with its table as literal text for both dtypes, the p-value, rank and
q-value expressions against scipy's recorded values (tests/golden/assoc_vectors.json), the relabellings, every argument and
groups-file rule, and the host module over the CPU double with the native writer against the sequential model."""
import json
import os

import numpy as np
import pytest

from midas_amd import abi, build
from midas_amd.analyze import cli, genes_assoc
from tests import compare_genes_model as CG
from tests import gene_assoc_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# six genes x seven samples: three cases (c1, c2, c3), three controls (k1, k2, k3) and x, which the groups file does not name
SAMPLES = ['c1', 'c2', 'k1', 'x', 'c3', 'k2', 'k3']
HAND = [('all_cases', '1.0 1.0 0.0 9.0 1.0 0.0 0.0'),       # in every case and no control
        ('tied', '0.5 2.0 0.5 0.0 2.0 0.5 0.0'),            # doubled midranks 6 11 6 . 11 6 2: w = 28, ties = 24 + 6
        ('equal', '1.5 1.5 1.5 0.0 1.5 1.5 1.5'),           # var = 0: p = 1, every relabelling is as extreme
        ('dropped', '0.0 0.1 0.0 5.0 0.2 0.0 0.3'),         # present in x only, which is not used: c = 0 < --min_present
        ('controls', '0.0 0.0 1.0 0.0 0.0 1.0 0.0'),
        ('mixed', '3.0 0.0 1.0 0.0 0.4 0.0 0.36')]
HAND_TEXT = '\t'.join(['gene_id'] + SAMPLES) + '\n' + ''.join(g + '\t' + v.replace(' ', '\t') + '\n' for g, v in HAND)
HAND_GROUPS = "# phenotype\nsample_id\tlabel\nc1\tsick\nk1\thealthy\nc2\tsick\n\nk2\thealthy\nc3\tsick\nk3\thealthy\nelsewhere\tsick\n"
# presabs, on paper: all_cases a = 3 of c = 3: the tables x = 0 and x = 3 have 1 / 20 each: p = 0.1, q = 0.1 * 5 / 1;
# controls a = 0 of c = 2: x = 0 and x = 2 have 3 / 15 each, x = 1 has 9 / 15: p = 0.4
HAND_PRESABS = ("gene_id\tcount_case\tcount_control\teffect\tp_value\tq_value\texceed\tp_perm\tq_perm\n"
                "all_cases\t3\t0\t1.0\t0.09999999999999996\t0.49999999999999983\t3\t0.19047619047619047\t0.7142857142857142\n"
                "tied\t3\t2\t0.33333333333333337\t1.0\t1.0\t20\t1.0\t1.0\n"
                "equal\t3\t3\t0.0\t1.0\t1.0\t20\t1.0\t1.0\n"
                "controls\t0\t2\t-0.6666666666666666\t0.39999999999999925\t0.9999999999999981\t5\t0.2857142857142857\t0.7142857142857142\n"
                "mixed\t2\t2\t0.0\t0.999999999999999\t1.0\t20\t1.0\t1.0\n")
# copynum, on paper: all_cases has ranks 10 10 4 . 10 4 4: w = 30, ties = 2 * (27 - 3), U1 = 15 - 6 = 9, var = 0.75 * (7 - 48 / 30)
# = 4.05, z = 4 / sqrt(4.05) = 1.98762, p = erfc(z / sqrt 2) = 0.046854; effect = 9 / 9
HAND_COPYNUM = ("gene_id\tcount_case\tcount_control\teffect\tp_value\tq_value\texceed\tp_perm\tq_perm\n"
                "all_cases\t3\t0\t1.0\t0.046854177603873774\t0.23427088801936888\t3\t0.19047619047619047\t0.6349206349206349\n"
                "tied\t3\t2\t0.8888888888888888\t0.15729920705028513\t0.3127205499914739\t7\t0.38095238095238093\t0.6349206349206349\n"
                "equal\t3\t3\t0.5\t1.0\t1.0\t20\t1.0\t1.0\n"
                "controls\t0\t2\t0.16666666666666666\t0.18763232999488436\t0.3127205499914739\t5\t0.2857142857142857\t0.6349206349206349\n"
                "mixed\t2\t2\t0.6111111111111112\t0.8247780950825133\t1.0\t17\t0.8571428571428571\t1.0\n")
HAND_ARGV = ['--permutations', '20', '--seed', '1']


def _dir(tmp_path, text, name='species_1'):
    return CG.write_dir(str(tmp_path / name), text)


def _groups(tmp_path, text, name='groups.txt'):
    path = str(tmp_path / name)
    with open(path, 'w', newline='') as f:
        f.write(text)
    return path


def test_the_case_worked_by_hand_in_the_model():
    table, res = M.model_tables(HAND_TEXT, HAND_GROUPS, dict(permutations=20, seed=1))
    assert table == HAND_PRESABS
    assert (res['n_used'], res['n_case'], res['n_kept']) == (6, 3, 5) and res['row_of_slot'].tolist() == [0, 1, 2, 4, 5]
    assert res['count'].tolist() == [3, 5, 6, 2, 4] and res['w'].tolist() == [3, 3, 3, 0, 2] and not res['ties'].any()
    table, res = M.model_tables(HAND_TEXT, HAND_GROUPS, dict(dtype='copynum', permutations=20, seed=1))
    assert table == HAND_COPYNUM
    assert res['w'].tolist() == [30, 28, 21, 15, 23] and res['ties'].tolist() == [48, 30, 6 ** 3 - 6, 66, 6]
    assert res['exceed'][2] == 20 and (res['products'][2] == 21).all()
    assert abs(float(HAND_PRESABS.split('\n')[1].split('\t')[4]) - 0.1) < 1e-15 and abs(float(HAND_PRESABS.split('\n')[4].split('\t')[4]) - 0.4) < 1e-14
    # without relabellings the last three columns are not written
    assert M.model_tables(HAND_TEXT, HAND_GROUPS, {})[0].split('\n')[1] == "all_cases\t3\t0\t1.0\t0.09999999999999996\t0.49999999999999983"


@pytest.mark.parametrize("dtype,table", [('presabs', HAND_PRESABS), ('copynum', HAND_COPYNUM)])
def test_the_host_module_and_the_native_writer_write_the_hand_case(tmp_path, dtype, table):
    d, g = _dir(tmp_path, HAND_TEXT), _groups(tmp_path, HAND_GROUPS)
    printed, got = M.run(d, g, HAND_ARGV + ['--dtype', dtype], str(tmp_path / 'out.txt'), M.ModelContext)
    assert got == table
    for line in ("Samples used: 6 (3 of the case group sick, 3 of the control group healthy)", "Samples of the matrix without a label, left out: 1",
                 "Rows read: 6", "Genes kept (present in >= 1 and absent from >= 0 of 6 samples): 5", "Relabellings of the samples: 20 (seed 1)"):
        assert line in printed.split('\n'), (line, printed)
    # --case turns the signs of the effects round and leaves the p-values
    printed, got = M.run(d, g, ['--dtype', dtype, '--case', 'healthy'], str(tmp_path / 'out.txt'), M.ModelContext)
    assert got == M.model_tables(HAND_TEXT, HAND_GROUPS, dict(dtype=dtype, case='healthy'))[0]
    assert [r.split('\t')[4] for r in got.split('\n')[1:-1]] == [r.split('\t')[4] for r in table.split('\n')[1:-1]]
    assert got.split('\n')[1].split('\t')[:4] == ['all_cases', '0', '3', '-1.0' if dtype == 'presabs' else '0.0']


def test_the_expressions_against_scipys_recorded_values():
    with open(os.path.join(ROOT, 'tests', 'golden', 'assoc_vectors.json')) as f:
        vec = json.load(f)
    worst = vec['worst_rel_diff']
    assert max(worst.values()) < 1e-9
    rel = lambda a, b: 0.0 if a == b else abs(a - b) / max(abs(a), abs(b))
    assert len(vec['fisher']) >= 200 and len(vec['ranksum']) >= 36 and max(len(c['label']) for c in vec['ranksum']) == 1000
    sizes = set()
    for a, c, n1, n2, p in vec['fisher']:
        sizes.add((n1, n2))
        lf = genes_assoc.log_factorials(n1 + n2)
        assert rel(genes_assoc.fisher_p(a, c, n1, n2, lf), p) <= 10 * worst['fisher'], (a, c, n1, n2)
        assert rel(M.fisher(a, c, n1, n2), p) <= 10 * worst['fisher'], (a, c, n1, n2)
    assert (1, 1) in sizes and (400, 600) in sizes
    heavy = equal = 0
    for case in vec['ranksum']:
        index, label = np.array([int(k) for k in case['index']]), np.array([int(ch) for ch in case['label']])
        r2, T = M.midranks(np.array(case['levels'])[index])
        assert r2.tolist() == np.array(case['ranks2'])[index].tolist() and T == case['ties']        # exactly scipy's ranks, doubled
        n1 = int(label.sum())
        n2 = label.shape[0] - n1
        w = int(r2[label == 1].sum())
        heavy += T > 0.5 * (label.shape[0] ** 3 - label.shape[0])
        for U1, p in (genes_assoc.ranksum_p(w, T, n1, n2), M.ranksum(w, T, n1, n2)):
            if case['p'] is None:
                equal += 1
                assert p == 1.0 and T == label.shape[0] ** 3 - label.shape[0]
            else:
                assert U1 == case['U1'] and rel(p, case['p']) <= 10 * worst['ranksum']
    assert heavy >= 5 and equal >= 5
    for case in vec['bh']:
        for q in (genes_assoc.benjamini_hochberg(case['p']).tolist(), M.bh(case['p'])):
            assert len(q) == len(case['q']) and all(rel(x, y) <= 10 * worst['bh'] for x, y in zip(q, case['q']))
        assert genes_assoc.benjamini_hochberg(case['p']).tolist() == M.bh(case['p'])


def test_the_relabellings():
    used = [1, 3, 4, 64, 66, 127, 128, 130]
    planes = genes_assoc.permutation_planes(used, 3, 50, 7, 131)
    assert planes.dtype == np.uint64 and planes.shape == (50, 3)
    mask = genes_assoc.words_of(used, 131)
    assert all(sum(bin(int(w)).count('1') for w in plane) == 3 for plane in planes)
    assert not (planes & ~mask).any()
    assert np.array_equal(planes, genes_assoc.permutation_planes(used, 3, 50, 7, 131))
    assert not np.array_equal(planes, genes_assoc.permutation_planes(used, 3, 50, 8, 131))
    assert np.array_equal(planes, M.planes_for(used, 3, 50, 7, 131))
    assert len({plane.tobytes() for plane in planes}) > 20                        # (56 subsets of 3 out of 8)
    assert genes_assoc.permutation_planes(used, 3, 0, 7, 131).shape == (0, 3)
    # the first plane is the first draw of numpy's generator
    first = np.random.default_rng(7).permutation(8)[:3]
    assert planes[0].tolist() == genes_assoc.words_of([used[k] for k in first], 131).tolist()


def _exit_of(argv):
    with pytest.raises(SystemExit) as ei:
        cli.gene_assoc_arguments(argv)
    code = str(ei.value.code)
    assert code.startswith("\nError: ") and code.endswith("\n")
    return code


def test_every_argument_error(tmp_path):
    d, g = _dir(tmp_path, HAND_TEXT), _groups(tmp_path, HAND_GROUPS)
    assert "Input file does not exist: %s/genes_presabs.txt" % str(tmp_path / 'nowhere') in _exit_of([str(tmp_path / 'nowhere'), '--groups', g])
    assert "--groups is required" in _exit_of([d])
    assert "Specified input file '%s' does not exist" % str(tmp_path / 'none.txt') in _exit_of([d, '--groups', str(tmp_path / 'none.txt')])
    assert "--min_present cannot be a negative number" in _exit_of([d, '--groups', g, '--min_present', '-1'])
    assert "--min_absent cannot be a negative number" in _exit_of([d, '--groups', g, '--min_absent', '-1'])
    assert "--permutations must be between 0 and 1000000" in _exit_of([d, '--groups', g, '--permutations', '-1'])
    assert "--permutations must be between 0 and 1000000" in _exit_of([d, '--groups', g, '--permutations', '1000001'])
    assert "--seed cannot be a negative number" in _exit_of([d, '--groups', g, '--seed', '-1'])
    assert "--cutoff must be a finite number" in _exit_of([d, '--groups', g, '--cutoff', 'nan'])
    assert "--group_rows cannot be a negative number" in _exit_of([d, '--groups', g, '--group_rows', '-1'])
    assert "--chunk_bytes cannot be a negative number" in _exit_of([d, '--groups', g, '--chunk_bytes', '-1'])
    assert "--form must be 0 or 1" in _exit_of([d, '--groups', g, '--form', '2'])
    args = cli.gene_assoc_arguments([d, '--groups', g])
    want = dict(out='/dev/stdout', case=None, max_genes=None, max_samples=None, dtype='presabs', cutoff=0.35, min_present=1, min_absent=0,
                permutations=0, seed=0, group_rows=0, chunk_bytes=0, form=1)
    assert {k: args[k] for k in want} == want
    assert cli.gene_assoc_arguments([d, '--groups', g, '--permutations', '1000000'])['permutations'] == 1000000
    with pytest.raises(SystemExit) as ei:
        cli.gene_assoc_arguments(['-h'])
    assert ei.value.code == 0


def test_every_rule_of_the_groups_file(tmp_path):
    d = _dir(tmp_path, HAND_TEXT)

    def exit_of(groups_text, options=()):
        g = _groups(tmp_path, groups_text)
        with pytest.raises(SystemExit) as ei:
            M.run(d, g, list(options), str(tmp_path / 'out.txt'), M.ModelContext)
        code = str(ei.value.code)
        assert code.startswith("\nError: %s" % g) and code.endswith("\n")
        return code
    assert ", line 4: the sample c1 has the label healthy here and sick on line 1" in exit_of("c1\tsick\nk1\thealthy\n\nc1\thealthy\n")
    assert ", line 3: a third label, other, beside sick and healthy" in exit_of("c1\tsick\nk1\thealthy\nc2\tother\n")
    assert ": two groups are needed, but the samples of the matrix carry the label sick only" in exit_of("c1\tsick\nc2\tsick\nelsewhere\thealthy\n")
    assert ": two groups are needed, but the samples of the matrix carry no label" in exit_of("# nothing\nelsewhere\tsick\n")
    assert ": --case other: no sample of the matrix has this label" in exit_of(HAND_GROUPS, ['--case', 'other'])
    assert ", line 2: not sample_id<TAB>label" in exit_of("c1\tsick\nk1 healthy\n")
    # a third label on a sample the matrix does not have, the same label twice and a label only --max_samples cuts off are no errors
    g = _groups(tmp_path, HAND_GROUPS + "elsewhere2\tother\nc1\tsick\n")
    assert M.run(d, g, HAND_ARGV, str(tmp_path / 'out.txt'), M.ModelContext)[1] == HAND_PRESABS
    assert ": two groups are needed, but the samples of the matrix carry the label sick only" in exit_of(HAND_GROUPS, ['--max_samples', '2'])
    # more than 8 191 used samples
    ids = ['s%d' % k for k in range(8192)]
    wide = _dir(tmp_path, 'gene_id\t' + '\t'.join(ids) + '\ng\t' + '\t'.join(['1.0'] * 8192) + '\n', 'wide')
    g = _groups(tmp_path, ''.join('%s\t%s\n' % (id, 'ab'[k & 1]) for k, id in enumerate(ids)), 'wide.txt')
    with pytest.raises(SystemExit) as ei:
        M.run(wide, g, [], str(tmp_path / 'out.txt'), M.ModelContext)
    assert str(ei.value.code) == "\nError: %s: 8192 samples of the matrix carry a label, more than 8191\n" % g


def _random_matrix(n_genes, n_samples, seed):
    rng = np.random.default_rng(seed)
    spell = ('0.0', '0', '0.35', '0.36', '1.5', '2.25', '7e-1', '12', '0.21', '3.0')
    ids = ['sample%d' % s for s in range(n_samples)]
    rows = ['\t'.join(['gene_id'] + ids)]
    for g in range(n_genes):
        few = rng.integers(1, len(spell) + 1)
        rows.append('\t'.join(['gene_%d' % g] + [spell[k] for k in rng.integers(0, few, n_samples)]))
    label = {id: 'ab'[int(rng.integers(0, 2))] for id in ids if rng.random() < 0.8}
    return '\n'.join(rows) + '\n', ''.join('%s\t%s\n' % kv for kv in label.items())


@pytest.mark.parametrize("dtype", ['presabs', 'copynum'])
def test_the_host_module_over_the_double_writes_the_models_table(tmp_path, dtype):
    text, groups = _random_matrix(120, 30, seed=5)
    d, g = _dir(tmp_path, text), _groups(tmp_path, groups)
    for options, argv in ((dict(dtype=dtype), []),
                          (dict(dtype=dtype, permutations=64, seed=3, min_present=3, min_absent=2, cutoff=0.5, max_samples=25, max_genes=100, case='a'),
                           ['--permutations', '64', '--seed', '3', '--min_present', '3', '--min_absent', '2', '--cutoff', '0.5', '--max_samples', '25',
                            '--max_genes', '100', '--case', 'a'])):
        table, res = M.model_tables(text, groups, options)
        printed, got = M.run(d, g, ['--dtype', dtype] + argv, str(tmp_path / 'out.txt'), M.ModelContext)
        assert got == table
        assert 20 < res['n_kept'] <= res['n_rows'] and "Rows read: %d" % res['n_rows'] in printed.split('\n')
        cols = genes_assoc.table_columns(res)
        exp = M.columns(res)
        for k in exp:
            assert cols[k].dtype == np.float64 and cols[k].tolist() == exp[k], k
    assert res['n_kept'] < res['n_rows'] == 100 and res['n_used'] < 25 and res['exceed'].min() < 64


def test_a_matrix_without_a_kept_gene_writes_the_header_alone(tmp_path):
    text = '\t'.join(['gene_id'] + SAMPLES) + '\nnone\t' + '\t'.join(['0.0'] * 7) + '\n'
    printed, got = M.run(_dir(tmp_path, text), _groups(tmp_path, HAND_GROUPS), HAND_ARGV, str(tmp_path / 'out.txt'), M.ModelContext)
    assert got == "gene_id\tcount_case\tcount_control\teffect\tp_value\tq_value\texceed\tp_perm\tq_perm\n"
    assert "Genes kept (present in >= 1 and absent from >= 0 of 6 samples): 0" in printed


def test_every_new_symbol_is_declared_bound_and_built():
    with open(os.path.join(ROOT, 'include', 'midas_snps.h')) as f:
        header = f.read()
    lib = abi.load_library()
    for name in ('midas_genes_assoc', 'midas_genes_assoc_write'):
        assert 'int32_t %s(' % name in header and name in abi.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert hasattr(abi.Context, 'genes_assoc') and hasattr(abi.GenesMatrix, 'write_assoc')
    assert 'genes_assoc.hip' in build.SOURCES and 'assoc_kernels.h' in build.HEADERS and 'genes_assoc.hip' not in build.SOURCE_FLAGS
    with open(os.path.join(ROOT, 'midas_amd', 'csrc', 'assoc_kernels.h')) as f:
        assert '__builtin_amdgcn_mfma_i32_16x16x64_i8' in f.read()
