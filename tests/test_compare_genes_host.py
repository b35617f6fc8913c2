"""compare_genes.py without a GPU: the sequential model against the reference's own output, the converter model against
pandas.read_table, the host module over a CPU double of the device (every golden table and progress line, byte for byte), the
error exits and the usage screen."""
import io
import os
import random
import struct
import subprocess
import sys

import numpy as np
import pytest

from midas_amd import abi
from midas_amd.analyze import cli, genes_compare, synth
from tests import compare_genes_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VEC = M.load_vectors()
CASES = list(range(len(VEC['cases'])))
EDGE = ['0', '1', '0.0', '1e5', '1E-5', '123456789012345678901234', '0.000000000000000000001234567890123456789', '1.', '.5', '+3.25',
        '-2.5e-3', '1e308', '1.7976931348623157e308', '2.2250738585072014e-308', '4.9e-324', '1e-400',
        '123456789.123456789123456789e-320', ' 7.5', '7.5 ', '00012.5', '1e+07', '9007199254740993', '0.1e1', '-0.0']
NOT_NUMBERS = ['', 'NA', 'nan', 'NaN', 'inf', '-inf', 'Infinity', 'abc', '1e', '1e400', '--1', '1.5x', '1 2', 'e5', '.', '1_0']


def bits(x):
    return struct.pack('<d', x)


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return M.write_tree(str(tmp_path_factory.mktemp("compare_genes")), VEC)


@pytest.mark.parametrize("k", CASES)
def test_the_model_writes_the_references_bytes(k):
    case = VEC['cases'][k]
    assert M.model_table(VEC['dirs'][case['dir']], M.case_options(case)) == M.case_table(case)


@pytest.mark.parametrize("k", CASES)
def test_the_host_module_over_the_model_writes_the_references_bytes_and_prints_its_lines(tree, tmp_path, k):
    case = VEC['cases'][k]
    printed, table = M.run(tree[case['dir']], case['options'], str(tmp_path / 'out.txt'), M.ModelContext)
    assert table == M.case_table(case)
    assert printed == case['printed']


def test_the_golden_covers_what_it_must():
    seen = {(M.case_options(c).get('dtype', 'presabs'), M.case_options(c).get('distance', 'jaccard')) for c in VEC['cases']}
    assert len(seen) == 6
    opts = [M.case_options(c) for c in VEC['cases']]
    assert any(o.get('max_genes') == 0 for o in opts) and any(o.get('max_samples') == 0 for o in opts)
    assert any(o.get('max_genes', 0) > 0 for o in opts) and any(o.get('max_samples', 0) > 1 for o in opts)
    assert {o.get('cutoff') for o in opts} >= {0.1, 0.75}
    widths = {len(t.split('\n')[0].split('\t')) - 1 for t in VEC['dirs'].values()}
    assert 3 in widths and 130 in widths
    assert any(row.split('\t')[5:] == ['0', '0'] for c in VEC['cases'] if not c['options'] or c['options'][0] == '--cutoff'
               for row in M.case_table(c).split('\n')[1:] if row)       # a sample with no gene present: count_either 0 -> 0
    cells = [cell for t in VEC['dirs'].values() for line in t.split('\n')[1:] if line for cell in line.split('\t')[1:]]
    differ = sum(M.pandas_float(c)[0] != float(c) for c in cells)
    assert differ * 10 >= len(cells), (differ, len(cells))
    assert any('e-' in c for c in cells) and any('e+' in c or float(c) > 1e6 for c in cells)
    # correctly rounded parsing would write other copynum lines
    case = next(c for c in VEC['cases'] if c['dir'] == 'six' and c['options'] == ['--dtype', 'copynum', '--distance', 'jaccard'])
    real = M.pandas_float
    M.pandas_float = lambda c: (float(c), True)
    try:
        rounded = M.model_table(VEC['dirs']['six'], M.case_options(case))
    finally:
        M.pandas_float = real
    assert rounded != M.case_table(case)


def test_the_converter_model_and_the_library_equal_pandas_read_table():
    pd = pytest.importorskip('pandas')
    rng = random.Random(20241016)
    cells = [repr(rng.random() * rng.choice([1, 1, 1, 10, 100, 1e-7, 1e7, 1e-3, 1e-300, 1e300])) for _ in range(100000)]
    cells += ['%.6g' % (rng.random() * 50) for _ in range(2000)] + EDGE
    got = pd.read_table(io.StringIO('x\n' + '\n'.join(cells) + '\n'))['x'].values
    assert got.dtype == np.float64 and got.shape[0] == len(cells)
    differ = 0
    for cell, want in zip(cells, got):
        model, lib = M.pandas_float(cell), abi.pandas_cell(cell.encode())
        assert model is not None and lib is not None, cell
        assert bits(model[0]) == bits(float(want)) and bits(lib[0]) == bits(float(want)) and model[1] == lib[1], cell
        differ += model[0] != float(cell)
    assert differ > 10000                       # this is not float()
    six = ['%.6g' % (rng.random() * 50) for _ in range(5000)]
    assert all(M.pandas_float(c)[0] == float(c) for c in six)


@pytest.mark.parametrize("cell", NOT_NUMBERS)
def test_cells_that_are_no_finite_decimal_literal(cell):
    assert M.pandas_float(cell) is None and abi.pandas_cell(cell.encode()) is None


def test_plain_integers_are_told_from_decimals():
    for cell, plain in [('3', True), ('-12', True), (' 4', True), ('3.0', False), ('3.', False), ('3e0', False), ('.5', False)]:
        assert M.pandas_float(cell)[1] == plain and abi.pandas_cell(cell.encode())[1] == plain


def test_numpys_cumsum_is_the_interpreters_sum():
    rng = np.random.default_rng(7)
    x = rng.gamma(2.0, 0.6, (5000, 3)) * rng.choice([1.0, 1e-7, 1e7], (5000, 3))
    for c in range(3):
        assert bits(float(M.ordered_sum(x)[c])) == bits(float(sum(x[:, c])))
    pairwise = float(np.sum(x[:, 0]))
    assert bits(pairwise) != bits(float(sum(x[:, 0])))          # (a tree of additions gives other bits: the order is the result)


def test_the_synthetic_directory_is_what_the_command_reads(tmp_path):
    d = str(tmp_path / 'species_1')
    info = synth.write_genes_dir(d, 700, 9, seed=3, block=256)
    text = open(os.path.join(d, 'genes_copynum.txt')).read()
    assert text.split('\n')[0].split('\t') == ['gene_id'] + info['sample_ids'] and text.count('\n') == 701
    cells = [c for line in text.split('\n')[1:] if line for c in line.split('\t')[1:]]
    assert sum(len(c) >= 17 for c in cells) * 2 > len(cells) and sum(M.pandas_float(c)[0] != float(c) for c in cells) * 10 > len(cells)
    for options in (['--dtype', 'copynum', '--distance', 'euclidean'], ['--cutoff', '0.75']):
        printed, table = M.run(d, options, str(tmp_path / 'out.txt'), M.ModelContext)
        assert table == M.model_table(text, M.case_options(dict(options=options)))


# ---- the exits ----------------------------------------------------------------------------------------------------------------
def _exit_of(indir, options, tmp_path):
    with pytest.raises(SystemExit) as ei:
        M.run(indir, options, str(tmp_path / 'out.txt'), M.ModelContext)
    return str(ei.value.code)


def _edited(tmp_path, edit):
    rows = [r.split('\t') for r in VEC['dirs']['three'].split('\n')[:-1]]
    edit(rows)
    return M.write_dir(str(tmp_path / 'edited'), '\n'.join('\t'.join(r) for r in rows) + '\n')


def test_a_missing_input_file_exits_with_the_references_text(tmp_path):
    with pytest.raises(SystemExit) as ei:
        cli.compare_genes_arguments([str(tmp_path / 'nowhere')])
    assert str(ei.value.code) + '\n' == VEC['missing']['stderr'].replace('<TMP>', str(tmp_path))
    d = M.write_dir(str(tmp_path / 'd'), VEC['dirs']['three'])
    os.unlink(os.path.join(d, 'genes_depth.txt'))
    with pytest.raises(SystemExit) as ei:
        cli.compare_genes_arguments([d])
    assert str(ei.value.code) == "\nError: Input file does not exist: %s/genes_depth.txt\n" % d


def test_header_exits(tmp_path):
    d = _edited(tmp_path, lambda rows: rows[0].__setitem__(0, 'cluster'))
    assert "genes_copynum.txt, line 1: the first column is 'cluster', not gene_id" in _exit_of(d, [], tmp_path)
    d = _edited(tmp_path, lambda rows: rows[0].__setitem__(3, rows[0][1]))
    assert "line 1: the sample id s000 names columns 2 and 4" in _exit_of(d, [], tmp_path)
    d = M.write_dir(str(tmp_path / 'plain'), VEC['dirs']['three'])
    assert "--max_samples 4, but the matrix has 3 sample columns" in _exit_of(d, ['--max_samples', '4'], tmp_path)
    assert "--max_genes cannot be a negative number" in _exit_of(d, ['--max_genes', '-1'], tmp_path)


def test_a_duplicate_beyond_max_samples_is_not_read(tmp_path):
    d = _edited(tmp_path, lambda rows: rows[0].__setitem__(3, rows[0][1]))
    printed, table = M.run(d, ['--max_samples', '2'], str(tmp_path / 'out.txt'), M.ModelContext)
    assert len(table.split('\n')) == 3


@pytest.mark.parametrize("cell", ['', 'NA', 'nan', 'inf', 'text', '1e999'])
def test_a_cell_that_is_no_number_exits_with_file_line_and_column(tmp_path, cell):
    d = _edited(tmp_path, lambda rows: rows[41].__setitem__(2, cell))
    msg = _exit_of(d, ['--dtype', 'copynum'], tmp_path)
    assert "genes_copynum.txt, line 42, column 3 (sample s001): the cell is not a finite decimal number" in msg
    assert "line 42" in _exit_of(d, [], tmp_path)
    printed, table = M.run(d, ['--max_samples', '1'], str(tmp_path / 'out.txt'), M.ModelContext)       # the column is not in use
    assert table.count('\n') == 1
    printed, table = M.run(d, ['--max_genes', '40'], str(tmp_path / 'out.txt'), M.ModelContext)        # nor is the row
    assert table.count('\n') == 4


def test_a_row_of_another_width_exits_and_the_earliest_error_wins(tmp_path):
    d = _edited(tmp_path, lambda rows: rows[30].append('0.5'))
    assert "genes_copynum.txt, line 31: the row does not have 3 sample columns" in _exit_of(d, [], tmp_path)
    d = _edited(tmp_path, lambda rows: rows[30].pop())
    assert "line 31: the row does not have 3 sample columns" in _exit_of(d, [], tmp_path)

    def both(rows):
        rows[30].pop()
        rows[12][3] = 'NA'
        rows[12][1] = 'x'
    assert "line 13, column 2 (sample s000)" in _exit_of(_edited(tmp_path, both), [], tmp_path)


def test_a_column_of_plain_integers_is_refused_under_copynum_alone(tmp_path):
    def ints(rows):
        for r in rows[1:]:
            r[2] = str(int(float(r[2])))
    d = _edited(tmp_path, ints)
    msg = _exit_of(d, ['--dtype', 'copynum'], tmp_path)
    assert "genes_copynum.txt, column 3 (sample s001): no cell has a decimal point or an exponent" in msg
    printed, table = M.run(d, [], str(tmp_path / 'out.txt'), M.ModelContext)
    assert table == M.model_table(open(os.path.join(d, 'genes_copynum.txt')).read(), {})


def test_usage_screen():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'compare_genes.py'), '-h'], capture_output=True, text=True,
                       env=dict(os.environ, COLUMNS='80'))
    assert r.returncode == 0
    ours, theirs = r.stdout.split('\n'), VEC['usage'].split('\n')
    assert ours[0] == theirs[0] == 'Description:' and 'Usage: compare_genes.py indir [options]' in ours
    assert '--group_rows' not in r.stdout and not any(line.startswith('usage:') for line in ours)
    # every option line of the reference's screen: the same flags, metavars and choices, and the same default in parentheses
    for line in theirs:
        if line.startswith('  -') or line.startswith('  PATH'):
            head = line[:24].rstrip() if len(line) > 24 and line[22:24] == '  ' else line.rstrip()
            assert any(o.startswith(head) for o in ours), line
    for default in ('(jaccard)', '(presabs)', '(0.35)', '(all)'):
        assert default in r.stdout
    assert 'Examples:' in ours


def test_every_new_symbol_is_declared_and_bound():
    header = open(os.path.join(ROOT, 'include', 'midas_snps.h')).read()
    lib = abi.load_library()
    for sym in ('midas_genes_matrix_open', 'midas_genes_matrix_counts', 'midas_genes_matrix_columns', 'midas_genes_matrix_close',
                'midas_genes_compare_parse_cell', 'midas_genes_compare', 'midas_genes_compare_write_pairs'):
        assert sym + '(' in header and sym in abi.EXPORTED_SYMBOLS and getattr(lib, sym).argtypes is not None
    assert '#define MIDAS_SNPS_ABI_VERSION 4' in header and abi.ABI_VERSION == 4
