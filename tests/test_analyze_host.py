"""snp_diversity.py / call_consensus.py without a GPU: the native readers against csv, the sequential model of the device call
against the reference's own output (tests/golden/analyze_vectors.json), the model's pairwise mean against np.mean bit for bit,
and both command lines with the model injected through run_pipeline's make_context: output bytes, argument block, every
check_args exit, the --rand_reads message and the file-and-line message for malformed cells."""
import contextlib
import csv
import io
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

from midas_amd import abi
from midas_amd.analyze import cli, consensus, diversity, sites
from tests import analyze_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VEC = M.load_vectors()


def _write_species(d, sp):
    os.makedirs(d, exist_ok=True)
    for k in ('summary', 'info', 'freq', 'depth'):
        with open('%s/snps_%s.txt' % (d, k), 'w', newline='') as f:
            f.write(sp[k])


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("analyze"))
    for name, sp in VEC['species'].items():
        _write_species('%s/%s' % (tmp, name), sp)
    for name, text in VEC['site_lists'].items():
        with open('%s/%s.list' % (tmp, name), 'w') as f:
            f.write(text)
    return tmp


def _argv(tree, case, out):
    opts = ['%s/%s.list' % (tree, o) if o in VEC['site_lists'] else o for o in case['options']]
    return ['%s/%s' % (tree, case['species'])] + opts + ['--out', out]


def _run(script, tree, case, out, make_context=M.ModelContext):
    argv = _argv(tree, case, out)
    parse, check, pipeline = (cli.diversity_arguments, cli.check_diversity_args, diversity.run_pipeline) if script == 'snp_diversity.py' else \
        (cli.consensus_arguments, cli.check_consensus_args, consensus.run_pipeline)
    args = parse(argv)
    check(args)
    buf = io.StringIO()
    saved = sys.argv
    sys.argv = [script] + argv
    try:
        with contextlib.redirect_stdout(buf):
            cli.print_args(args, script)
            if case.get('seed') is not None:
                random.seed(case['seed'])
            pipeline(args, make_context=make_context)
    finally:
        sys.argv = saved
    return buf.getvalue()


def _rows(text, per_gene):
    lines = text.split('\n')
    return [lines[0]] + sorted(lines[1:]) if per_gene else lines


def check_diversity_case(tree, case, out, make_context=M.ModelContext):
    printed = _run('snp_diversity.py', tree, case, out, make_context)
    per_gene = 'per-gene' in case['options']
    assert _rows(open(out).read(), per_gene) == _rows(case['out'], per_gene)
    block = case['args_block'].replace('<TMP>', tree).replace('%s/out.txt' % tree, out)
    assert printed.startswith(block)
    assert " %d samples selected" % case['n_samples'] in printed


def check_consensus_case(tree, case, out, make_context=M.ModelContext):
    printed = _run('call_consensus.py', tree, case, out, make_context)
    assert open(out).read() == case['out']
    assert printed == case['args_block'].replace('<TMP>', tree).replace('%s/out.txt' % tree, out)


@pytest.mark.parametrize("k", range(len(VEC['diversity'])))
def test_snp_diversity_with_the_model_writes_the_references_bytes(tree, tmp_path, k):
    check_diversity_case(tree, VEC['diversity'][k], str(tmp_path / 'pi.txt'))


@pytest.mark.parametrize("k", range(len(VEC['consensus'])))
def test_call_consensus_with_the_model_writes_the_references_bytes(tree, tmp_path, k):
    check_consensus_case(tree, VEC['consensus'][k], str(tmp_path / 'seqs.fa'))


def test_every_sites_symbol_is_declared_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "midas_snps.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(midas_sites_[a-z_0-9]+)\s*\(", src)))
    assert declared == sorted(abi.SITES_SYMBOLS) and len(declared) >= 6
    lib = abi.load_library()
    for sym in declared:
        assert getattr(lib, sym).argtypes is not None, sym
    from midas_amd import build
    assert 'sites_scan.hip' in build.SOURCES and 'sites_io.cpp' in build.SOURCES and 'text_numbers.h' in build.HEADERS
    assert '-ffp-contract=off' in build.SOURCE_FLAGS['sites_scan.hip']
    # the row walker and the site step are headers: an edit rebuilds, and every file that compiles a copy keeps one rounding
    assert 'sites_rows.h' in build.HEADERS and 'sites_call.h' in build.HEADERS
    users = [s for s in build.SOURCES
             if re.search(r'#include "sites_(rows|call)\.h"', open(os.path.join(ROOT, 'midas_amd', 'csrc', s), errors='replace').read())]
    assert {'sites_scan.hip', 'sites_strains.hip', 'sites_trees.hip'} <= set(users)
    for s in users:
        assert '-ffp-contract=off' in build.SOURCE_FLAGS.get(s, []), s


def test_the_golden_covers_what_it_must():
    opts = [' '.join(c['options']) for c in VEC['diversity']]
    for need in ('per-gene', 'pooled-samples', '--weight_by_depth', '--consensus', '--site_prev', '--site_maf', '--site_ratio',
                 '--allele_support', '--site_type 4D', '--max_sites', 'in_order', 'out_of_order', '--rand_sites', '--sample_depth',
                 '--keep_samples', '--exclude_samples', '--max_samples'):
        assert any(need in o for o in opts), need
    assert any('--consensus' in o and 'per-gene' in o and 'pooled' in o for o in opts)
    n = {k: len(v['summary'].splitlines()) - 1 for k, v in VEC['species'].items()}
    assert max(n.values()) > 128 and any(9 <= x <= 20 for x in n.values())
    small = VEC['species']['small']
    assert '\tN\t' in small['info'] and all(('\t%s\t' % c) in small['freq'] or ('\t%s\n' % c) in small['freq'] for c in ('0', '1', '0.5', '0.0123', '1e-05'))
    cells = [c for row in small['freq'].splitlines()[1:] for c in row.split('\t')[1:]]
    assert any(not M.is_fast_float(c) for c in cells) and sum(M.is_fast_float(c) for c in cells) > 0.9 * len(cells)
    rag = VEC['species']['ragged']
    assert len(rag['depth'].splitlines()) < len(rag['freq'].splitlines())


def test_pairwise_mean_is_numpys_mean_bit_for_bit():
    rng = np.random.default_rng(3)
    bad = 0
    for n in range(1, 301):
        for _ in range(12):
            v = (rng.random(n) * 10.0 ** rng.integers(-3, 3, n)).tolist() if n % 2 else rng.random(n).tolist()
            a, b = M.pairwise_mean(v), float(np.mean(v))
            bad += a != b and not (a != a and b != b)
    assert bad == 0
    left = lambda v: sum(v[1:], v[0]) / len(v)
    v9 = [rng.random(9).tolist() for _ in range(400)]
    assert any(left(v) != float(np.mean(v)) for v in v9)        # a left-to-right sum is NOT np.mean from 9 values on


def test_readers_match_csv(tree):
    for name in VEC['species']:
        d = '%s/%s' % (tree, name)
        t = abi.SitesTables(d)
        summary = list(csv.DictReader(open(d + '/snps_summary.txt'), delimiter='\t'))
        assert t.strings('sample_id') == [r['sample_id'] for r in summary]
        assert t.mean_coverage.tolist() == [float(r['mean_coverage']) for r in summary]
        assert t.fraction_covered.tolist() == [float(r['fraction_covered']) for r in summary]
        info = list(csv.DictReader(open(d + '/snps_info.txt'), delimiter='\t'))
        for col in ('site_id', 'ref_allele', 'major_allele', 'minor_allele', 'locus_type', 'site_type'):
            assert t.strings(col) == [r[col] for r in info], col
        genes = []
        for r in info:
            if r['gene_id'] != '' and r['gene_id'] not in genes:
                genes.append(r['gene_id'])
        assert t.strings('gene_id') == genes
        assert t.gene.tolist() == [genes.index(r['gene_id']) if r['gene_id'] else -1 for r in info]
        header = next(csv.reader(open(d + '/snps_depth.txt'), delimiter='\t'))
        assert t.strings('matrix_sample_id') == header[1:] and t.n_columns == len(header) - 1
        body = open(d + '/snps_freq.txt', newline='').read()
        assert t.freq_text.tobytes().decode() == body[body.index('\n') + 1:]
        assert t.equals('locus_type', 'CDS').tolist() == [r['locus_type'] == 'CDS' for r in info]


def test_reader_errors_name_file_and_line(tmp_path):
    sp = dict(VEC['species']['ragged'])
    lines = sp['summary'].splitlines()
    lines[2] = lines[2].rsplit('\t', 1)[0] + '\tabc'
    sp['summary'] = '\n'.join(lines) + '\n'
    _write_species(str(tmp_path / 'a'), sp)
    with pytest.raises(abi.MidasSnpsError) as e:
        abi.SitesTables(str(tmp_path / 'a'))
    assert 'snps_summary.txt, line 3' in e.value.message
    with pytest.raises(abi.MidasSnpsError) as e:
        abi.SitesTables(str(tmp_path / 'missing'))
    assert 'snps_summary.txt' in e.value.message


def test_host_cell_parser_is_float_and_int():
    for c in ['0.5', ' 0.5 ', '1_0.5', '1e400', '1e-400', 'nan', '-inf', 'Infinity', '.5', '5.', '0.12345678901234567890', '4.9e-324', '1__0',
              '_1', '1_', '', 'abc', '0x10', '1e', '--1']:
        try:
            exp = float(c)
        except ValueError:
            exp = None
        got = abi.parse_cell(c.encode(), 'freq')
        assert (got is None) == (exp is None) and (exp is None or got == exp or (got != got and exp != exp)), c
    for c in ['12', ' 12 ', '1_2', '+7', '-3', '007', '1.0', '', 'a', '1__2', '9223372036854775807']:
        try:
            exp = int(c)
        except ValueError:
            exp = None
        assert abi.parse_cell(c.encode(), 'depth') == exp, c


CHECKS = [
    (['--site_depth', '1'], "--site_depth must be >=2 to calculate nucleotide variation"),
    (['--max_sites', '0'], "--max_sites must be >= 1 to calculate nucleotide variation"),
    (['--max_samples', '0'], "--max_samples must be >= 1 to calculate nucleotide variation"),
    (['--site_ratio', '-1'], "--site_ratio cannot be a negative number"),
    (['--sample_depth', '-1'], "--sample_depth cannot be a negative number"),
    (['--site_maf', '1.5'], "--site_maf must be between 0 and 1"),
    (['--site_prev', '-0.1'], "--site_prev must be between 0 and 1"),
    (['--sample_cov', '2'], "--fract_cov must be between 0 and 1"),
    (['--rand_sites', '1.5'], "--rand_sites must be between 0 and 1"),
    (['--genomic_type', 'per-gene'], "--locus_type must be CDS if --genomic_type is per-gene"),
    (['--site_type', '4D'], "--locus_type must be CDS if --site_type is specified"),
    (['--rand_reads', '5'], "--rand_reads / --replace_reads are not part of this build"),
    (['--replace_reads'], "--rand_reads / --replace_reads are not part of this build"),
]


@pytest.mark.parametrize("opts, message", CHECKS)
def test_snp_diversity_check_args_exits(tree, opts, message):
    args = cli.diversity_arguments(['%s/small' % tree] + opts)
    with pytest.raises(SystemExit) as e:
        cli.check_diversity_args(args)
    assert e.value.code == "\nError: %s\n" % message


def test_other_exits(tree, tmp_path):
    with pytest.raises(SystemExit) as e:
        cli.check_diversity_args(cli.diversity_arguments([str(tmp_path / 'nowhere')]))
    assert "Specified input directory '%s' does not exist" % (tmp_path / 'nowhere') in e.value.code
    with pytest.raises(SystemExit) as e:
        cli.check_consensus_args(cli.consensus_arguments(['%s/small' % tree, '--site_depth', '0']))
    assert e.value.code == "\nError: --site_depth must be >=1\n"
    for opts in (['--sample_depth', '1000'], ):
        with pytest.raises(SystemExit) as e:
            _run('snp_diversity.py', tree, dict(species='small', options=opts), str(tmp_path / 'o'))
        assert "no samples satisfied your selection criteria" in e.value.code
    with pytest.raises(SystemExit) as e:
        _run('snp_diversity.py', tree, dict(species='small', options=['--rand_samples', '100']), str(tmp_path / 'o'))
    assert "--rand_samples cannot exceed the number of samples" in e.value.code
    # the scripts themselves start and stop before the device is touched
    for script in ('snp_diversity.py', 'call_consensus.py'):
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', script), str(tmp_path / 'nowhere')], stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, text=True)
        assert r.returncode != 0 and "does not exist" in r.stderr
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', script), '-h'], stdout=subprocess.PIPE, text=True)
        assert r.returncode == 0 and '--site_prev' in r.stdout and '--max_sites' in r.stdout


def test_rand_samples_picks_numpys_choice_in_file_order(tree):
    t = sites.open_tables('%s/small' % tree)
    np.random.seed(5)
    got = sites.fetch_samples(t, rand_samples=5)
    np.random.seed(5)
    exp = set(np.random.choice(t.strings('sample_id'), 5, replace=False).tolist())
    assert set(got) == exp and list(got) == [s for s in t.strings('sample_id') if s in exp]


@pytest.mark.parametrize("which, cell, what", [('freq', '0.5x', 'not a number'), ('freq', '', 'not a number'), ('depth', '3.0', 'not an integer')])
def test_malformed_cells_exit_with_file_and_line(tmp_path, which, cell, what):
    sp = dict(VEC['species']['ragged'])
    rows = sp[which].split('\n')
    f = rows[7].split('\t')
    f[3] = cell
    rows[7] = '\t'.join(f)
    sp[which] = '\n'.join(rows)
    d = str(tmp_path / 'ragged')
    _write_species(d, sp)
    for script in ('snp_diversity.py', 'call_consensus.py'):
        with pytest.raises(SystemExit) as e:
            _run(script, str(tmp_path), dict(species='ragged', options=[]), str(tmp_path / 'o'))
        assert e.value.code == "\nError: %s/snps_%s.txt, line 8: sample s002: the cell is %s\n" % (d, which, what)
    # a short row
    f[3] = '3'
    rows[7] = '\t'.join(f[:5])
    sp[which] = '\n'.join(rows)
    _write_species(d, sp)
    with pytest.raises(SystemExit) as e:
        _run('snp_diversity.py', str(tmp_path), dict(species='ragged', options=[]), str(tmp_path / 'o'))
    assert e.value.code == "\nError: %s/snps_%s.txt, line 8: the row has fewer sample columns than the samples in use\n" % (d, which)
    # ... which a run that stops before the row never sees
    _run('snp_diversity.py', str(tmp_path), dict(species='ragged', options=['--max_sites', '2']), str(tmp_path / 'o'))


def test_call_consensus_with_alleles_that_are_not_one_letter(tmp_path):
    """'NA' alleles (a site no sample covers, as merge_midas.py snps --all_sites writes them): '-' where nothing is kept, the
    two letters where a sample is -- fetch_consensus appends the allele string whatever its length."""
    sp = dict(VEC['species']['ragged'])
    rows = sp['info'].split('\n')
    for k in (2, 6):            # site 2: covered; site 6 (index 5): depth 0 everywhere
        f = rows[k].split('\t')
        f[4] = f[5] = 'NA'
        rows[k] = '\t'.join(f)
    sp['info'] = '\n'.join(rows)
    _write_species(str(tmp_path / 'ragged'), sp)
    out = str(tmp_path / 'seq.fa')
    _run('call_consensus.py', str(tmp_path), dict(species='ragged', options=[]), out)
    got = open(out).read().splitlines()
    exp = [c for c in VEC['consensus'] if c['species'] == 'ragged' and not c['options']][0]['out'].splitlines()
    assert len(got) == len(exp)
    longer = 0
    for g, e in zip(got[1::2], exp[1::2]):
        assert len(g) - len(e) == g.count('NA')
        assert g.count('-') == e.count('-')
        longer += g.count('NA')
    assert longer > 0
    assert all(('length=%d ' % len(s)) in h for h, s in zip(got[0::2], got[1::2]))
