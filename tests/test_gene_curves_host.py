"""gene_curves.py without a device: the sequential model on a case worked by hand, the product's need[] against a linear
search, the orders table against numpy's generator, every argument and --samples error, both tables as the native writers
write them, the Heaps fit, and the new symbols."""
import math
import os

import numpy as np
import pytest

from midas_amd import abi, build
from midas_amd.analyze import cli, genes_curves, synth
from tests import compare_genes_model as CG
from tests import gene_curves_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLES = ['s0', 's1', 's2', 's3', 's4']
# six genes x five samples: a gene of every sample, one that misses the last sample, one of two samples in the middle, one of
# the last sample alone, one of the last two, and one of no sample
HAND = [('core', '11111'), ('most', '11110'), ('half', '01100'), ('lone', '00001'), ('late', '00011'), ('none', '00000')]
HAND_TEXT = M.matrix_text([g for g, _ in HAND], SAMPLES, [[ch == '1' for ch in bits] for _, bits in HAND])
HAND_ORDERS = [[0, 1, 2, 3, 4], [4, 3, 2, 1, 0]]


def _dir(tmp_path, text, name='species_1'):
    return CG.write_dir(str(tmp_path / name), text)


def _hand(core_frac):
    _, cells = M.split_matrix(HAND_TEXT, {})
    return M.curves(cells, 0.35, HAND_ORDERS, M.need_linear(5, core_frac))


def test_the_case_worked_by_hand():
    # the counts c(g, r, k) along the listed order and along its reverse
    #   order 0   core 1 2 3 4 5   most 1 2 3 4 4   half 0 1 2 2 2   lone 0 0 0 0 1   late 0 0 0 1 2   none 0 0 0 0 0
    #   order 1   core 1 2 3 4 5   most 0 1 2 3 4   half 0 0 1 2 2   lone 1 1 1 1 1   late 1 2 2 2 2   none 0 0 0 0 0
    assert M.need_linear(5, 1.0) == [0, 1, 2, 3, 4, 5]
    res = _hand(1.0)
    assert res['pan'].tolist() == [[2, 3, 3, 4, 5], [3, 4, 5, 5, 5]]
    assert res['core'].tolist() == [[2, 2, 2, 2, 1], [3, 2, 1, 1, 1]]
    assert res['single'].tolist() == [[2, 1, 0, 1, 1], [3, 2, 2, 1, 1]]
    assert all(res[k].dtype == np.int64 for k in ('pan', 'core', 'single'))
    # at 0.75 three of four and four of five are enough: `most` stays core in order 0 and comes back in order 1
    assert M.need_linear(5, 0.75) == [0, 1, 2, 3, 3, 4]
    soft = _hand(0.75)
    assert soft['pan'].tolist() == res['pan'].tolist() and soft['single'].tolist() == res['single'].tolist()
    assert soft['core'].tolist() == [[2, 2, 2, 2, 2], [3, 2, 1, 2, 2]]
    assert M.curves_text(soft) == (
        "samples\tpan\tcore\tsingle\tnew\tpan_mean\tpan_min\tpan_max\tcore_mean\tcore_min\tcore_max\tsingle_mean\tsingle_min\tsingle_max\tnew_mean\n"
        "1\t2\t2\t2\t2\t3.0\t3\t3\t3.0\t3\t3\t3.0\t3\t3\t3.0\n"
        "2\t3\t2\t1\t1\t4.0\t4\t4\t2.0\t2\t2\t2.0\t2\t2\t1.0\n"
        "3\t3\t2\t0\t0\t5.0\t5\t5\t1.0\t1\t1\t2.0\t2\t2\t1.0\n"
        "4\t4\t2\t1\t1\t5.0\t5\t5\t2.0\t2\t2\t1.0\t1\t1\t0.0\n"
        "5\t5\t2\t1\t1\t5.0\t5\t5\t2.0\t2\t2\t1.0\t1\t1\t0.0\n")
    one = {k: res[k][:1] for k in ('pan', 'core', 'single')}
    assert M.curves_text(one) == "samples\tpan\tcore\tsingle\tnew\n1\t2\t2\t2\t2\n2\t3\t2\t1\t1\n3\t3\t2\t0\t0\n4\t4\t2\t1\t1\n5\t5\t1\t1\t1\n"
    assert M.orders_text(SAMPLES, res, HAND_ORDERS).split('\n')[5:8] == ["0\t5\ts4\t5\t1\t1", "1\t1\ts4\t3\t3\t3", "1\t2\ts3\t4\t2\t2"]


def test_the_native_writers_write_the_hand_case(tmp_path):
    m = abi.GenesMatrix(os.path.join(_dir(tmp_path, HAND_TEXT), 'genes_copynum.txt'))
    soft = _hand(0.75)
    out = str(tmp_path / 'c.txt')
    m.write_curves(out, soft, genes_curves.table_columns(soft))
    assert open(out).read() == M.curves_text(soft)
    m.write_curve_orders(out, soft, HAND_ORDERS)
    assert open(out).read() == M.orders_text(SAMPLES, soft, HAND_ORDERS)
    one = {k: soft[k][:1] for k in ('pan', 'core', 'single')}
    m.write_curves(out, one, genes_curves.table_columns(one))
    assert open(out).read() == M.curves_text(one)
    with pytest.raises(abi.MidasSnpsError):
        m.write_curve_orders(out, soft, [[0, 1, 2, 3, 5], [4, 3, 2, 1, 0]])      # no sixth column
    with pytest.raises(abi.MidasSnpsError) as ei:
        m.write_curves(str(tmp_path / 'nowhere' / 'c.txt'), soft, genes_curves.table_columns(soft))
    assert "cannot be written" in ei.value.message


@pytest.mark.parametrize("t", [0.5, 0.95, math.nextafter(0.95, 1.0), 1.0])
def test_need_by_bisection_is_need_by_linear_search(t):
    need = genes_curves.need_table(200, t)
    assert need.dtype == np.int32 and need.tolist() == M.need_linear(200, t)
    assert need[0] == 0 and all(1 <= need[k] <= k for k in range(1, 201))


def test_need_at_its_borders():
    assert genes_curves.need_table(64, 1.0).tolist() == list(range(65))
    assert float(19) / float(20) == 0.95
    assert genes_curves.need_table(20, 0.95)[19:].tolist() == [19, 19]
    assert genes_curves.need_table(20, math.nextafter(0.95, 1.0))[20] == 20
    assert genes_curves.need_table(8, 1e-9).tolist() == [0] + [1] * 8           # never 0: a gene of no sample is not core


def test_the_orders_table():
    used = [0, 2, 3, 5, 8, 9]
    orders = genes_curves.orders_table(used[::-1], 4, 11)
    assert orders.dtype == np.int32 and orders.shape == (5, 6) and orders[0].tolist() == used
    rng = np.random.default_rng(11)
    for r in range(1, 5):
        assert orders[r].tolist() == [used[j] for j in rng.permutation(6)]
    assert np.array_equal(orders, M.orders_model(used, 4, 11))
    assert not np.array_equal(orders[1:], genes_curves.orders_table(used, 4, 12)[1:])
    assert genes_curves.orders_table(used, 0, 11).tolist() == [used]


def _exit_of(argv):
    with pytest.raises(SystemExit) as ei:
        cli.gene_curves_arguments(argv)
    code = str(ei.value.code)
    assert code.startswith("\nError: ") and code.endswith("\n")
    return code


def test_every_argument_error(tmp_path):
    d = _dir(tmp_path, HAND_TEXT)
    assert "Input file does not exist: %s/genes_presabs.txt" % str(tmp_path / 'nowhere') in _exit_of([str(tmp_path / 'nowhere')])
    assert "Specified input file '%s' does not exist" % str(tmp_path / 'ids.txt') in _exit_of([d, '--samples', str(tmp_path / 'ids.txt')])
    assert "--cutoff must be a finite number" in _exit_of([d, '--cutoff', 'inf'])
    for bad in ('0', '-0.5', '1.0000001', 'nan'):
        assert "--core_frac must be above 0 and at most 1" in _exit_of([d, '--core_frac', bad])
    for bad in ('-1', '100001'):
        assert "--permutations must be between 0 and 100000" in _exit_of([d, '--permutations', bad])
    assert "--seed cannot be a negative number" in _exit_of([d, '--seed', '-1'])
    assert "--group_rows cannot be a negative number" in _exit_of([d, '--group_rows', '-1'])
    assert "--chunk_bytes cannot be a negative number" in _exit_of([d, '--chunk_bytes', '-1'])
    assert "--form must be 0 or 1" in _exit_of([d, '--form', '2'])
    args = cli.gene_curves_arguments([d])
    want = dict(out='/dev/stdout', orders=None, samples=None, max_genes=None, max_samples=None, cutoff=0.35, core_frac=1.0, permutations=100,
                seed=0, group_rows=0, chunk_bytes=0, form=1)
    assert {k: args[k] for k in want} == want
    assert cli.gene_curves_arguments([d, '--permutations', '100000'])['permutations'] == 100000
    with pytest.raises(SystemExit) as ei:
        cli.gene_curves_arguments(['-h'])
    assert ei.value.code == 0


def _run_exit(d, options, tmp_path):
    with pytest.raises(SystemExit) as ei:
        M.run(d, options, str(tmp_path / 'out.txt'))
    code = str(ei.value.code)
    assert code.startswith("\nError: ") and code.endswith("\n")
    return code


def test_the_samples_file(tmp_path):
    d = _dir(tmp_path, HAND_TEXT)
    ids = str(tmp_path / 'ids.txt')
    with open(ids, 'w') as f:
        f.write("# the samples of the second visit\ns3\tsecond\n\ns1\n   \ns3\ns0\textra\tfields\r\n")
    printed, table, orders = M.run(d, ['--samples', ids, '--permutations', '3', '--seed', '5'], str(tmp_path / 'c.txt'), str(tmp_path / 'o.txt'))
    exp_table, exp_orders, res = M.model_tables(HAND_TEXT, dict(permutations=3, seed=5), sample_lines=open(ids).read().split('\n'))
    assert res['orders'][0].tolist() == [0, 1, 3] and table == exp_table and orders == exp_orders
    assert "Samples in use: 3 of 5" in printed.split('\n')
    # without s2 and s4: core and most at 1 2 3, half at 0 1 1, late at 0 0 1
    assert res['pan'][0].tolist() == [2, 3, 4] and orders.split('\n')[3] == "0\t3\ts3\t4\t2\t2"
    with open(ids, 'w') as f:
        f.write("s1\ns2\n\nsample_9\n")
    assert "%s, line 4: the sample sample_9 is not among the 5 sample columns in use" % ids in _run_exit(d, ['--samples', ids], tmp_path)
    with open(ids, 'w') as f:
        f.write("s1\ns4\n")
    assert "%s, line 2: the sample s4 is not among the 4 sample columns in use" % ids in _run_exit(d, ['--samples', ids, '--max_samples', '4'], tmp_path)
    with open(ids, 'w') as f:
        f.write("# nobody\n\n")
    assert "%s: names no sample" % ids in _run_exit(d, ['--samples', ids], tmp_path)


def test_more_samples_than_the_widest_counter_holds(tmp_path):
    n = genes_curves.MAX_USED + 1
    text = M.matrix_text(['x'], ['s%d' % k for k in range(n)], [[True] * n])
    d = _dir(tmp_path, text)
    assert "8192 samples are in use, more than 8191: use --max_samples or --samples" in _run_exit(d, ['--permutations', '0'], tmp_path)
    printed, table, _ = M.run(d, ['--permutations', '0', '--max_samples', '8191'], str(tmp_path / 'c.txt'))
    assert table.count('\n') == 8192 and table.endswith("8191\t1\t1\t0\t0\n")


def test_the_rules_of_compare_genes_hold_for_the_matrix(tmp_path):
    rows = [r.split('\t') for r in HAND_TEXT.split('\n')[:-1]]
    d = _dir(tmp_path, HAND_TEXT)
    assert "--max_samples 6, but the matrix has 5 sample columns" in _run_exit(d, ['--max_samples', '6'], tmp_path)
    assert "--max_genes cannot be a negative number" in _run_exit(d, ['--max_genes', '-1'], tmp_path)
    rows[4][2] = 'NA'
    rows[5].append('1.5')
    d = _dir(tmp_path, '\n'.join('\t'.join(r) for r in rows) + '\n', 'bad')
    assert "genes_copynum.txt, line 5, column 3 (sample s1): the cell is not a finite decimal number" in _run_exit(d, [], tmp_path)
    assert "genes_copynum.txt, line 6: the row does not have 5 sample columns" in _run_exit(d, ['--max_samples', '1'], tmp_path)
    rows[0][0] = 'cluster'
    d = _dir(tmp_path, '\n'.join('\t'.join(r) for r in rows) + '\n', 'header')
    assert "line 1: the first column is 'cluster', not gene_id" in _run_exit(d, [], tmp_path)


def test_both_tables_on_a_synthetic_directory_byte_for_byte(tmp_path):
    d = str(tmp_path / 'species_1')
    info = synth.write_pangenome_curve_dir(d, 400, 40, seed=3)
    assert sorted(set(info['kind'].tolist())) == list(range(8))
    with open(os.path.join(d, 'genes_copynum.txt')) as f:
        text = f.read()
    _, cells = M.split_matrix(text, {})
    count = (cells > 0.35).sum(axis=0)
    for kind, lo, hi in ((0, 40, 40), (1, 39, 39), (2, 33, 40), (3, 15, 38), (4, 2, 25), (5, 0, 6), (6, 1, 1), (7, 0, 0)):
        c = count[info['kind'] == kind]
        assert c.size and lo <= c.min() and c.max() <= hi, kind
    for options, argv in ((dict(), []),
                          (dict(permutations=0), ['--permutations', '0']),
                          (dict(core_frac=0.95, permutations=7, seed=3, cutoff=0.5, max_genes=350, max_samples=33),
                           ['--core_frac', '0.95', '--permutations', '7', '--seed', '3', '--cutoff', '0.5', '--max_genes', '350', '--max_samples', '33'])):
        exp_table, exp_orders, res = M.model_tables(text, options)
        printed, table, orders = M.run(d, argv, str(tmp_path / 'c.txt'), str(tmp_path / 'o.txt'))
        assert table == exp_table and orders == exp_orders
        for line in res['lines']:
            assert line in printed.split('\n'), (line, printed)
        N = res['pan'].shape[1]
        # the input is not trivial: a core that is neither nothing nor everything, singletons, and orders that differ
        assert any(0 < res['core'][0][k] < res['pan'][0][k] for k in range(N)) and res['single'].max() > 0
        assert res['pan'].shape[0] == 1 or not np.array_equal(res['pan'][1], res['pan'][2])
        assert table.split('\n')[0].count('\t') == (4 if options.get('permutations') == 0 else 14)
    # a mean is str() of a quotient of an integer sum, a soft core is not monotone somewhere
    exp_table, _, res = M.model_tables(text, dict(core_frac=0.95, permutations=7, seed=3))
    line = exp_table.split('\n')[20].split('\t')
    assert line[5] == str(float(int(res['pan'][1:, 19].sum())) / 7.0) and line[6] == str(res['pan'][1:, 19].min())
    assert abi.format_repr_f64([1.0 / 7.0, 3.0, 0.25]) == [repr(1.0 / 7.0), '3.0', '0.25']


def test_the_heaps_fit(tmp_path):
    new = [round(1e6 * k ** -0.7) for k in range(1, 201)]
    alpha, K, is_open = genes_curves.heaps_fit(new)
    assert abs(alpha - 0.7) < 1e-3 and is_open and abs(K / 1e6 - 1) < 1e-2
    assert genes_curves.heaps_line(new) == M.heaps_line(new) and genes_curves.heaps_line(new).endswith(": open")
    closed = [round(1e9 * k ** -1.5) for k in range(1, 101)]
    assert genes_curves.heaps_line(closed).endswith(": closed") and abs(genes_curves.heaps_fit(closed)[0] - 1.5) < 1e-3
    assert genes_curves.heaps_fit([5, 0, 3, 0]) is None and genes_curves.heaps_fit([7]) is None           # one point, none
    assert genes_curves.heaps_fit([0, 4, 0, 2])[0] == pytest.approx(1.0)                                   # k = 1 is never a point
    # identical samples add nothing after the first one
    text = M.matrix_text(['a', 'b', 'c'], SAMPLES, [[True] * 5, [False] * 5, [True] * 5])
    printed, table, _ = M.run(_dir(tmp_path, text), ['--permutations', '4'], str(tmp_path / 'c.txt'))
    assert "Heaps' law: not fitted" in printed.split('\n')
    assert "All 5 samples: pan 2, core 2 (present in >= 5), single 0" in printed.split('\n')
    assert table.split('\n')[2] == "2\t2\t2\t0\t0\t2.0\t2\t2\t2.0\t2\t2\t0.0\t0\t0\t0.0"


def test_every_new_symbol_is_declared_and_bound():
    with open(os.path.join(ROOT, 'include', 'midas_snps.h')) as f:
        header = f.read()
    lib = abi.load_library()
    for name in ('midas_genes_curves', 'midas_genes_curves_write'):
        assert 'int32_t %s(' % name in header and name in abi.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert '#define MIDAS_SNPS_ABI_VERSION 4 ' in header and abi.ABI_VERSION == 4 and lib.midas_snps_abi_version() == 4
    assert callable(abi.genes_curves) and not hasattr(abi.Context, 'genes_curves')
    assert hasattr(abi.GenesMatrix, 'write_curves') and hasattr(abi.GenesMatrix, 'write_curve_orders')
    assert 'genes_curves.hip' in build.SOURCES and 'genes_curves.hip' not in build.SOURCE_FLAGS
    with open(os.path.join(ROOT, 'midas_amd', 'csrc', 'genes_curves.hip')) as f:
        source = f.read()
    assert '#include "genes_rows.h"' in source and 'planes_by_sample_kernel<1, PresentCell>' in source
    with open(os.path.join(ROOT, 'scripts', 'gene_curves.py')) as f:
        assert 'need[k]' in f.read()
