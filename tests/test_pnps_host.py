"""snp_pnps.py without a GPU: the command with the sequential model of the classed device call (tests/pnps_model.py) injected
through run_pipeline's make_context.  Each block of its output, projected, is the file the reference's snp_diversity.py wrote
for that site class (tests/golden/pnps_vectors.json), byte for byte; pnps is Python's division of the two printed pi_bp; the
argument block, every check_pnps_args exit, the options the parser refuses, --max_sites, and the new symbol's hygiene."""
import contextlib
import io
import os
import re
import sys

import numpy as np
import pytest

from midas_amd import abi
from midas_amd.analyze import cli, pnps, sites
from tests import analyze_model as AM
from tests import pnps_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AVEC = AM.load_vectors()
VEC = M.load_vectors()
CASES = VEC['cases']
BLOCK = ['sites', 'snps', 'pi', 'snps_kb', 'pi_bp']


def write_tree(tmp):
    for name, sp in AVEC['species'].items():
        os.makedirs('%s/%s' % (tmp, name), exist_ok=True)
        for k in ('summary', 'info', 'freq', 'depth'):
            with open('%s/%s/snps_%s.txt' % (tmp, name, k), 'w', newline='') as f:
                f.write(sp[k])
    for name, text in AVEC['site_lists'].items():
        with open('%s/%s.list' % (tmp, name), 'w') as f:
            f.write(text)
    return tmp


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return write_tree(str(tmp_path_factory.mktemp("pnps")))


def argv_of(tree, case, out):
    opts = ['%s/%s.list' % (tree, o) if o in AVEC['site_lists'] else o for o in case['options']]
    seed = [] if case.get('seed') is None else ['--seed', str(case['seed'])]
    return ['%s/%s' % (tree, case['species'])] + opts + seed + ['--out', out]


def run(tree, case, out, make_context=M.ModelContext):
    argv = argv_of(tree, case, out)
    args = cli.pnps_arguments(argv)
    cli.check_pnps_args(args)
    buf = io.StringIO()
    saved = sys.argv
    sys.argv = ['snp_pnps.py'] + argv
    try:
        with contextlib.redirect_stdout(buf):
            cli.print_args(args, 'snp_pnps.py')
            res = pnps.run_pipeline(args, make_context=make_context)
    finally:
        sys.argv = saved
    return buf.getvalue(), res


def table(text):
    rows = [ln.split('\t') for ln in text.split('\n') if ln != '']
    return rows[0], rows[1:]


def project(text, name):
    """The output with the other class's columns and pnps dropped and the _<class> suffix stripped."""
    header, rows = table(text)
    pick = [k for k, h in enumerate(header) if h.endswith('_' + name) or (h != 'pnps' and not any(h.endswith('_' + c) for c in pnps.CLASSES))]
    strip = lambda h: h[:-len(name) - 1] if h.endswith('_' + name) else h
    return ''.join('\t'.join(r) + '\n' for r in [[strip(header[k]) for k in pick]] + [[r[k] for k in pick] for r in rows])


def sorted_rows(text, per_gene):
    lines = text.split('\n')
    return [lines[0]] + sorted(lines[1:]) if per_gene else lines


def check_case(tree, case, out, make_context=M.ModelContext):
    printed, _ = run(tree, case, out, make_context)
    got = open(out).read()
    per_gene = 'per-gene' in case['options']
    for name in pnps.CLASSES:
        assert sorted_rows(project(got, name), per_gene) == sorted_rows(case['out_' + name], per_gene), name
    assert " %d samples selected" % case['n_samples'] in printed
    check_ratio(got)
    return got


def check_ratio(text):
    """pnps is float(pi_bp_1D) / float(pi_bp_4D) as repr() prints it; NA where either is NA or the divisor is 0.0."""
    header, rows = table(text)
    a, b, r = header.index('pi_bp_1D'), header.index('pi_bp_4D'), header.index('pnps')
    assert r == len(header) - 1
    n_na = 0
    for row in rows:
        if row[a] == 'NA' or row[b] == 'NA' or float(row[b]) == 0.0:
            assert row[r] == 'NA', row
            n_na += 1
        else:
            assert row[r] == repr(float(row[a]) / float(row[b])), row
    return n_na, len(rows)


@pytest.mark.parametrize("k", range(len(CASES)))
def test_each_block_is_the_references_snp_diversity_file(tree, tmp_path, k):
    check_case(tree, CASES[k], str(tmp_path / 'pnps.txt'))


def test_the_header(tree, tmp_path):
    for opts, lead in (([], ['sample_id', 'depth_1D']), (['--genomic_type', 'per-gene'], ['sample_id', 'gene_id', 'depth_1D']),
                       (['--sample_type', 'pooled-samples'], ['samples', 'sites_1D']),
                       (['--sample_type', 'pooled-samples', '--genomic_type', 'per-gene'], ['gene_id', 'samples', 'sites_1D'])):
        out = str(tmp_path / 'o.txt')
        run(tree, dict(species='small', options=opts), out)
        header, rows = table(open(out).read())
        block = lambda c: [n + '_' + c for n in ([] if 'samples' in lead else ['depth']) + BLOCK]
        assert header == lead[:-1] + block('1D') + block('4D') + ['pnps']
        assert all(len(r) == len(header) for r in rows)


def test_pnps_is_na_where_it_must_be(tree, tmp_path):
    """A gene without a 4D site (pi_bp_4D is NA), a per-sample --consensus run (every pi_bp is 0.0: NA by the zero divisor), and
    an ordinary run with numbers."""
    listed = [c for c in CASES if 'per-gene' in c['options'] and '--site_list' in c['options']][0]
    got = check_case(tree, listed, str(tmp_path / 'a.txt'))
    header, rows = table(got)
    no_4d = [r for r in rows if r[header.index('sites_4D')] == '0' and r[header.index('sites_1D')] != '0']
    assert no_4d and all(r[-1] == 'NA' and r[header.index('pi_bp_4D')] == 'NA' for r in no_4d)
    cons = [c for c in CASES if c['options'] == ['--consensus']][0]
    got = check_case(tree, cons, str(tmp_path / 'b.txt'))
    header, rows = table(got)
    assert all(r[-1] == 'NA' for r in rows) and any(r[header.index('pi_bp_4D')] == '0.0' for r in rows)
    assert all(r[header.index('pi_1D')] == '0' for r in rows)
    got = check_case(tree, CASES[0], str(tmp_path / 'c.txt'))
    n_na, n = check_ratio(got)
    assert n_na < n


def test_the_golden_covers_what_it_must():
    opts = [' '.join(c['options']) for c in CASES]
    assert len(CASES) >= 8
    for need in ('pooled-samples', 'per-gene', '--weight_by_depth', '--consensus', '--site_prev', '--site_maf', '--site_ratio', 'in_order',
                 '--rand_sites', '--keep_samples'):
        assert any(need in o for o in opts), need
    assert any('pooled' not in o for o in opts) and any('per-gene' not in o for o in opts)
    assert all(c['seed'] is not None for c in CASES if '--rand_sites' in c['options'])
    assert {c['species'] for c in CASES} == {'small', 'wide', 'ragged'} <= set(AVEC['species'])
    assert not any('--locus_type' in o or '--site_type' in o or '--max_sites' in o for o in opts)
    assert all(c['out_1D'] != c['out_4D'] for c in CASES)


def test_the_argument_block(tree, tmp_path):
    out = str(tmp_path / 'o.txt')
    case = dict(species='small', options=['--sample_type', 'pooled-samples', '--site_prev', '0.5'], seed=None)
    printed, _ = run(tree, case, out)
    exp = ["Command: snp_pnps.py %s" % ' '.join(argv_of(tree, case, out)), "Script: snp_pnps.py", "Input directory: %s/small" % tree,
           "Output file: %s" % out, "pN/pS options:", "  genomic_type: genome-wide", "  sample_type: pooled-samples", "  weight_by_depth: False",
           "  rand_samples: None", "  rand_sites: None", "  snp_maf: 0.01", "  consensus: False", "Sample filters:", "  sample_depth: 0.0",
           "  fract_cov: 0.0", "  max_samples: inf", "  keep_samples: None", "  exclude_samples: None", "Site filters:", "  site_list: None",
           "  site_depth: 2", "  site_prev: 0.5", "  site_maf: 0.0", "  site_ratio: inf", "  allele_support: 0.5", "  max_sites: inf"]
    assert printed.startswith('\n'.join(exp) + '\n')


CHECKS = [
    (['--site_depth', '1'], "--site_depth must be >=2 to calculate nucleotide variation"),
    (['--max_sites', '0'], "--max_sites must be >= 1 to calculate nucleotide variation"),
    (['--max_samples', '0'], "--max_samples must be >= 1 to calculate nucleotide variation"),
    (['--site_ratio', '-1'], "--site_ratio cannot be a negative number"),
    (['--site_depth', '-1'], "--site_depth must be >=2 to calculate nucleotide variation"),
    (['--sample_depth', '-1'], "--sample_depth cannot be a negative number"),
    (['--site_maf', '1.5'], "--site_maf must be between 0 and 1"),
    (['--site_prev', '-0.1'], "--site_prev must be between 0 and 1"),
    (['--sample_cov', '2'], "--fract_cov must be between 0 and 1"),
    (['--rand_sites', '1.5'], "--rand_sites must be between 0 and 1"),
]


@pytest.mark.parametrize("opts, message", CHECKS)
def test_check_pnps_args_exits(tree, opts, message):
    args = cli.pnps_arguments(['%s/small' % tree] + opts)
    with pytest.raises(SystemExit) as e:
        cli.check_pnps_args(args)
    assert e.value.code == "\nError: %s\n" % message


def test_other_exits_and_refused_options(tree, tmp_path, capsys):
    with pytest.raises(SystemExit) as e:
        cli.check_pnps_args(cli.pnps_arguments([str(tmp_path / 'nowhere')]))
    assert "Specified input directory '%s' does not exist" % (tmp_path / 'nowhere') in e.value.code
    cli.check_pnps_args(cli.pnps_arguments(['%s/small' % tree, '--genomic_type', 'per-gene']))          # (the classes are CDS sites)
    for opts in (['--locus_type', 'CDS'], ['--site_type', '4D'], ['--rand_reads', '5'], ['--replace_reads']):
        with pytest.raises(SystemExit) as e:
            cli.pnps_arguments(['%s/small' % tree] + opts)
        assert e.value.code == 2 and 'unrecognized arguments: %s' % opts[0] in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        run(tree, dict(species='small', options=['--sample_depth', '1000']), str(tmp_path / 'o'))
    assert "no samples satisfied your selection criteria" in e.value.code


def _class_inputs(tree, args):
    t = sites.open_tables(args['indir'])
    samples = sites.fetch_samples(t, args['sample_depth'], args['fract_cov'], args['max_samples'])
    mask, cls, n = pnps.class_mask(t, args)
    return t, samples, mask, cls, n


@pytest.mark.parametrize("n_max", [1, 7, 12])
def test_max_sites_counts_both_classes_together(tree, tmp_path, n_max):
    out = str(tmp_path / 'o.txt')
    case = dict(species='small', options=['--sample_type', 'pooled-samples', '--max_sites', str(n_max)])
    _, res = run(tree, case, out)
    header, rows = table(open(out).read())
    assert len(rows) == 1
    both = [int(rows[0][header.index('sites_' + c)]) for c in pnps.CLASSES]
    assert sum(both) == n_max == res['n_kept']
    assert n_max < 7 or min(both) > 0
    # the blocks are the model's: each class over its own sites among the rows up to the N-th retained one
    args = cli.pnps_arguments(argv_of(tree, case, out))
    t, samples, mask, cls, n = _class_inputs(tree, args)
    free = AM.sites_scan(t.freq_text, t.depth_text, mask[:n].astype(np.uint8), [s.index for s in samples.values()],
                         [s.mean_depth for s in samples.values()], 2, float('inf'), 0.5, 0.0, 0.0, flags=abi.SITES_SUMS | abi.SITES_POOLED, dump_keep=True)
    last = int(np.flatnonzero(free['keep'])[n_max - 1])
    for c, name in enumerate(pnps.CLASSES):
        m = (mask[:n] & (cls[:n] == c) & (np.arange(n) <= last)).astype(np.uint8)
        exp = AM.sites_scan(t.freq_text, t.depth_text, m, [s.index for s in samples.values()], [s.mean_depth for s in samples.values()], 2,
                            float('inf'), 0.5, 0.0, 0.0, flags=abi.SITES_SUMS | abi.SITES_POOLED)
        assert res['sites'][c, 0, 0] == exp['sites'][0, 0] == both[c] and res['snps'][c, 0, 0] == exp['snps'][0, 0]
        assert np.float64(res['pi'][c, 0, 0]).view(np.uint64) == np.float64(exp['pi'][0, 0]).view(np.uint64)
    # and differ from the separate runs', each of which stops at its own N-th site
    separate = [c for c in CASES if c['species'] == 'small' and c['options'] == ['--sample_type', 'pooled-samples']][0]
    if n_max == 7:
        assert project(open(out).read(), '1D') != separate['out_1D']


def test_rand_sites_draws_once_per_site_whatever_the_class(tree):
    """Under one seed the joint mask is the union of the two separate runs' masks."""
    import random
    from midas_amd.analyze import diversity
    t = sites.open_tables('%s/small' % tree)
    args = cli.pnps_arguments(['%s/small' % tree, '--rand_sites', '0.5'])
    random.seed(3)
    joint, cls, n = pnps.class_mask(t, args)
    for c, name in enumerate(pnps.CLASSES):
        random.seed(3)
        one, n1 = diversity.site_mask(t, dict(args, locus_type='CDS', site_type=name))
        assert n1 == n and np.array_equal(one, joint & (cls == c))
    assert 0 < joint.sum() < sites.info_mask(t, 'CDS', None).sum()


def test_the_model_refuses_what_the_device_refuses():
    none = np.zeros(0, np.uint8)
    text = np.frombuffer(b'1\t0.5\n2\t0.5\n', np.uint8)
    for cls, n, flags in (([0, 2], 2, abi.SITES_SUMS), ([0, 0], 0, abi.SITES_SUMS), ([0, 0], 5, abi.SITES_SUMS), ([0, 0], 2, abi.SITES_SEQ)):
        with pytest.raises(abi.MidasSnpsError) as e:
            M.sites_scan_classes(text, text, np.ones(2, np.uint8), np.array(cls, np.uint8), n, [0], [10.0], 2, float('inf'), 0.5, 0.0, 0.0, flags=flags)
        assert e.value.status == abi.ERR_INVALID_ARG
    assert none.size == 0


def test_the_new_symbol_is_declared_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "midas_snps.h")).read(), flags=re.S)
    assert re.search(r"\bmidas_sites_scan_classes\s*\(", src) and 'midas_sites_scan_classes' in abi.SITES_SYMBOLS
    assert '#define MIDAS_SITES_MAX_CLASSES %d' % abi.SITES_MAX_CLASSES in src
    lib = abi.load_library()
    assert getattr(lib, 'midas_sites_scan_classes').argtypes is not None
    assert len(lib.midas_sites_scan_classes.argtypes) == len(lib.midas_sites_scan.argtypes) + 2
    from midas_amd import build
    csrc = os.path.join(ROOT, 'midas_amd', 'csrc')
    homes = [s for s in build.SOURCES if 'midas_sites_scan_classes(' in open(os.path.join(csrc, s), errors='replace').read()]
    assert len(homes) == 1 and '-ffp-contract=off' in build.SOURCE_FLAGS.get(homes[0], [])
    text = open(os.path.join(csrc, homes[0])).read()
    assert text.count('rg.next(&g)') == 1                            # one group loop for every entry point
    assert text.count('hipLaunchKernelGGL(ss_sums_kernel,') == 1 and text.count('nullptr, 1, false)') == 2
    assert os.path.exists(os.path.join(ROOT, 'scripts', 'snp_pnps.py'))
