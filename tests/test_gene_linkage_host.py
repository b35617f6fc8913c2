"""gene_linkage.py without a device: the sequential model on a case worked by hand, the product's need[] against a linear
search, every argument error, the two tables as the native writers write them, and the header split genes_compare.hip went
through."""
import math
import os

import numpy as np
import pytest

from midas_amd import abi, build
from midas_amd.analyze import cli, genes_linkage, synth
from tests import compare_genes_model as CG
from tests import gene_linkage_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLES = ['s0', 's1', 's2', 's3', 's4']
# six genes x five samples: a core gene and a rare one that the filters drop, a chain a - b - c whose ends are not linked at
# T = 0.7 (a & b = b & c = 3 of 4, a & c = 3 of 5), and a gene that shares one sample with a and one with c
HAND = [('core', '11111'), ('a', '11110'), ('rare', '00001'), ('b', '01110'), ('c', '01111'), ('d', '10001')]
HAND_TEXT = M.matrix_text([g for g, _ in HAND], SAMPLES, [[ch == '1' for ch in bits] for _, bits in HAND])
HAND_OPTIONS = dict(min_jaccard=0.7, min_present=2, min_absent=1)


def _dir(tmp_path, text, name='species_1'):
    return CG.write_dir(str(tmp_path / name), text)


def test_the_case_worked_by_hand():
    assert M.need_linear(5, 0.7) == [0, 1, 2, 3, 3, 4]
    pairs, groups, res = M.model_tables(HAND_TEXT, HAND_OPTIONS)
    assert res['count'].tolist() == [4, 3, 4, 2] and res['row_of_slot'].tolist() == [1, 3, 4, 5]
    assert list(zip(res['pair_a'].tolist(), res['pair_b'].tolist(), res['pair_both'].tolist())) == [(0, 1, 3), (1, 2, 3)]
    assert res['label'].tolist() == [0, 0, 0, 3] and res['visited'] == 6 and res['linked'] == 2
    assert pairs == ("gene1\tgene2\tcount1\tcount2\tcount_both\tcount_either\tjaccard\n"
                     "a\tb\t4\t3\t3\t4\t0.75\n"
                     "b\tc\t3\t4\t3\t4\t0.75\n")
    assert groups == ("group_id\tgroup_size\tgene_id\tcount\n"
                      "1\t3\ta\t4\n1\t3\tb\t3\n1\t3\tc\t4\n")
    # at T = 0.6 the ends are linked too (3 of 5), and nothing else
    res = M.model_tables(HAND_TEXT, dict(HAND_OPTIONS, min_jaccard=0.6))[2]
    assert list(zip(res['pair_a'].tolist(), res['pair_b'].tolist())) == [(0, 1), (0, 2), (1, 2)]


def test_the_host_module_and_the_native_writers_write_the_hand_case(tmp_path):
    d = _dir(tmp_path, HAND_TEXT)
    printed, pairs, groups = M.run(d, ['--min_jaccard', '0.7', '--min_absent', '1'], str(tmp_path / 'p.txt'), str(tmp_path / 'g.txt'),
                                   M.ModelContext)
    exp_pairs, exp_groups, _ = M.model_tables(HAND_TEXT, HAND_OPTIONS)
    assert pairs == exp_pairs and groups == exp_groups
    for line in ("Rows read: 6", "Genes kept (present in >= 2 and absent from >= 1 of 5 samples): 4", "Pairs of genes visited: 6",
                 "Linked pairs (Jaccard index >= 0.7): 2", "Groups of at least 2 genes: 1"):
        assert line in printed.split('\n'), (line, printed)


@pytest.mark.parametrize("t", [0.5, 0.7, math.nextafter(0.7, 1.0), 0.9, 1.0])
def test_need_by_bisection_is_need_by_linear_search(t):
    assert genes_linkage.need_table(200, t).tolist() == M.need_linear(200, t)


def test_seven_of_ten_is_linked_at_point_seven_and_not_one_ulp_above():
    assert float(7) / float(10) == 0.7
    assert genes_linkage.need_table(10, 0.7)[10] == 7
    assert genes_linkage.need_table(10, math.nextafter(0.7, 1.0))[10] == 8
    assert genes_linkage.need_table(64, 1.0).tolist() == list(range(65))


def _exit_of(argv):
    with pytest.raises(SystemExit) as ei:
        cli.gene_linkage_arguments(argv)
    code = str(ei.value.code)
    assert code.startswith("\nError: ") and code.endswith("\n")
    return code


def test_every_argument_error(tmp_path):
    d = _dir(tmp_path, HAND_TEXT)
    assert "Input file does not exist: %s/genes_presabs.txt" % str(tmp_path / 'nowhere') in _exit_of([str(tmp_path / 'nowhere')])
    assert "--min_present must be >= 1" in _exit_of([d, '--min_present', '0'])
    assert "--min_absent cannot be a negative number" in _exit_of([d, '--min_absent', '-1'])
    for bad in ('0', '-0.5', '1.0000001', 'nan'):
        assert "--min_jaccard must be above 0 and at most 1" in _exit_of([d, '--min_jaccard', bad])
    assert "--min_group must be >= 2" in _exit_of([d, '--min_group', '1'])
    assert "--max_pairs must be between 0 and 2147483647" in _exit_of([d, '--max_pairs', '-1'])
    assert "--max_pairs must be between 0 and 2147483647" in _exit_of([d, '--max_pairs', str(1 << 31)])
    assert "--cutoff must be a finite number" in _exit_of([d, '--cutoff', 'inf'])
    assert "--group_rows cannot be a negative number" in _exit_of([d, '--group_rows', '-1'])
    assert "--chunk_bytes cannot be a negative number" in _exit_of([d, '--chunk_bytes', '-1'])
    args = cli.gene_linkage_arguments([d])
    want = dict(out='/dev/stdout', groups=None, max_genes=None, max_samples=None, cutoff=0.35, min_present=2, min_absent=2, min_jaccard=0.9,
                min_group=2, max_pairs=1 << 26, group_rows=0, chunk_bytes=0)
    assert {k: args[k] for k in want} == want
    with pytest.raises(SystemExit) as ei:
        cli.gene_linkage_arguments(['-h'])
    assert ei.value.code == 0


def test_the_rules_of_compare_genes_hold_for_the_matrix(tmp_path):
    def exit_of(d, options):
        with pytest.raises(SystemExit) as ei:
            M.run(d, options, str(tmp_path / 'out.txt'), None, M.ModelContext)
        return str(ei.value.code)
    rows = [r.split('\t') for r in HAND_TEXT.split('\n')[:-1]]
    d = _dir(tmp_path, HAND_TEXT)
    assert "--max_samples 6, but the matrix has 5 sample columns" in exit_of(d, ['--max_samples', '6'])
    assert "--max_genes cannot be a negative number" in exit_of(d, ['--max_genes', '-1'])
    rows[4][2] = 'NA'
    rows[5].append('1.5')
    d = _dir(tmp_path, '\n'.join('\t'.join(r) for r in rows) + '\n', 'bad')
    assert "genes_copynum.txt, line 5, column 3 (sample s1): the cell is not a finite decimal number" in exit_of(d, [])
    assert "genes_copynum.txt, line 6: the row does not have 5 sample columns" in exit_of(d, ['--max_samples', '1'])
    rows[0][0] = 'cluster'
    d = _dir(tmp_path, '\n'.join('\t'.join(r) for r in rows) + '\n', 'header')
    assert "line 1: the first column is 'cluster', not gene_id" in exit_of(d, [])


def test_more_pairs_than_max_pairs_exits_with_the_total_and_names_both_options(tmp_path):
    d = _dir(tmp_path, HAND_TEXT)
    with pytest.raises(SystemExit) as ei:
        M.run(d, ['--min_jaccard', '0.7', '--min_absent', '1', '--max_pairs', '1'], str(tmp_path / 'out.txt'), None, M.ModelContext)
    msg = str(ei.value.code)
    assert "2 pairs of genes are linked, more than --max_pairs 1" in msg and "--min_jaccard" in msg


def test_the_table_formats_on_a_synthetic_directory(tmp_path):
    d = str(tmp_path / 'species_1')
    info = synth.write_linked_genes_dir(d, 300, 40, seed=3, groups=[5, 9, 17])
    assert sorted(np.bincount(info['group_of'][info['group_of'] >= 0]).tolist()) == [5, 9, 17]
    with open(os.path.join(d, 'genes_copynum.txt')) as f:
        text = f.read()
    for options, argv in ((dict(min_jaccard=0.8), ['--min_jaccard', '0.8']),
                          (dict(min_jaccard=0.8, min_group=6, max_samples=33, max_genes=250),
                           ['--min_jaccard', '0.8', '--min_group', '6', '--max_samples', '33', '--max_genes', '250'])):
        exp_pairs, exp_groups, res = M.model_tables(text, options)
        printed, pairs, groups = M.run(d, argv, str(tmp_path / 'p.txt'), str(tmp_path / 'g.txt'), M.ModelContext)
        assert pairs == exp_pairs and groups == exp_groups
        assert 0 < res['linked'] < res['visited'] // 20
    # every planted group comes back as one component, and the jaccard column is repr() of a quotient
    exp_pairs, exp_groups, res = M.model_tables(text, dict(min_jaccard=0.8))
    slot_of = {int(r): k for k, r in enumerate(res['row_of_slot'])}
    for g in range(3):
        members = [slot_of[r] for r in np.flatnonzero(info['group_of'] == g) if r in slot_of]
        assert len(members) >= 4 and len({int(res['label'][k]) for k in members}) == 1
    assert all(repr(float(line.split('\t')[4]) / float(line.split('\t')[5])) == line.split('\t')[6] for line in exp_pairs.split('\n')[1:-1])
    assert abi.format_repr_f64([9.0 / 11.0, 1.0, 0.75]) == [repr(9.0 / 11.0), '1.0', '0.75']


def test_a_matrix_without_a_kept_gene_writes_the_headers_alone(tmp_path):
    text = M.matrix_text(['x', 'y'], SAMPLES, [[True] * 5, [False] * 5])
    printed, pairs, groups = M.run(_dir(tmp_path, text), [], str(tmp_path / 'p.txt'), str(tmp_path / 'g.txt'), M.ModelContext)
    assert pairs == "gene1\tgene2\tcount1\tcount2\tcount_both\tcount_either\tjaccard\n"
    assert groups == "group_id\tgroup_size\tgene_id\tcount\n"
    assert "Genes kept (present in >= 2 and absent from >= 2 of 5 samples): 0" in printed


def test_the_row_parser_moved_to_a_header_and_compare_genes_is_what_it_was(tmp_path):
    with open(os.path.join(ROOT, 'midas_amd', 'csrc', 'genes_compare.hip')) as f:
        compare = f.read()
    with open(os.path.join(ROOT, 'midas_amd', 'csrc', 'genes_rows.h')) as f:
        rows = f.read()
    with open(os.path.join(ROOT, 'midas_amd', 'csrc', 'genes_linkage.hip')) as f:
        linkage = f.read()
    assert '#include "genes_rows.h"' in compare and '#include "genes_rows.h"' in linkage
    for name in ('void gc_parse_kernel(', 'struct GcParseP {', 'struct midas_genes_matrix {'):
        assert name in rows and name not in compare and name not in linkage
    assert 'genes_rows.h' in build.HEADERS and 'genes_linkage.hip' in build.SOURCES and 'genes_linkage.hip' not in build.SOURCE_FLAGS
    # the command over the CPU double writes the reference's bytes for every golden case, as before the split
    vec = CG.load_vectors()
    tree = CG.write_tree(str(tmp_path / 'golden'), vec)
    for case in vec['cases']:
        printed, table = CG.run(tree[case['dir']], case['options'], str(tmp_path / 'out.txt'), CG.ModelContext)
        assert table == CG.case_table(case) and printed == case['printed']
    # and the library's host build of the converter, which the header's kernel calls, agrees with the model
    for cell in ('0', '0.35', '1e-5', '123456789012345678901234', '4.9e-324', '00012.5'):
        assert abi.pandas_cell(cell.encode()) == CG.pandas_float(cell)


def test_every_new_symbol_is_declared_and_bound():
    with open(os.path.join(ROOT, 'include', 'midas_snps.h')) as f:
        header = f.read()
    lib = abi.load_library()
    for name in ('midas_genes_linkage', 'midas_genes_linkage_write_pairs', 'midas_genes_linkage_write_groups'):
        assert 'int32_t %s(' % name in header and name in abi.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert hasattr(abi.Context, 'genes_linkage') and hasattr(abi.GenesMatrix, 'write_linkage') and hasattr(abi.GenesMatrix, 'write_groups')
    with open(os.path.join(ROOT, 'scripts', 'gene_linkage.py')) as f:
        assert 'need[either]' in f.read()
