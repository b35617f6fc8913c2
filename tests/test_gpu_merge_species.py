"""merge_species.py on the GPU box: every golden case (tests/golden/merge_species_vectors.json) in process and through the script,
the four files byte for byte; twelve species over N samples at the edges of numpy's pairwise reduce and of odd / even medians
against the sequential model (tests/merge_species_model.py) -- means, medians and their rounded values as bit patterns,
prevalence, order -- in LDS and, with the bound lowered, through the radix sort; groups of one and of several files and a file
larger than the chunk; every refusal this build adds, the earliest one named, at two chunk sizes; 600 species x 40 samples
through the script."""
import os
import subprocess
import sys

import numpy as np
import pytest

from midas_amd import abi
from midas_amd.merge import species as mspecies
from tests import merge_species_model as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VEC = M.load_vectors()
CASES = [c['name'] for c in VEC['cases']]
SEED = 20261018
NAMES = ('mean_coverage', 'median_coverage', 'mean_abundance', 'median_abundance')
HEAD = 'species_id\tcount_reads\tcoverage\trelative_abundance\n'


@pytest.fixture(scope="module")
def ctx():
    with abi.Context(0) as c:
        yield c


def bits(x):
    return np.asarray(x, np.float64).view(np.uint64).tolist()


def merged(ctx, root, ids, sample_ids, profiles, depth=1.0, **kw):
    paths = M.write_samples(str(root), sample_ids, profiles)
    return ctx.species_merge(paths, ids, depth, **kw)


def same(res, want):
    assert bits(res.coverage) == bits(want['coverage']) and bits(res.abundance) == bits(want['abundance'])
    assert res.reads.tolist() == want['reads']
    for n in NAMES:
        assert bits(getattr(res, n)) == bits(want[n]), n
        assert bits(res.rounded[n]) == bits(want['rounded'][n]), n
    assert res.prevalence.tolist() == want['prevalence'] and res.order.tolist() == want['order']


def files_of(res, out, sample_ids, threads=0):
    os.makedirs(str(out), exist_ok=True)
    res.write(str(out), sample_ids, threads)
    return dict((f, open(os.path.join(str(out), f)).read()) for f in M.FILES)


@pytest.mark.parametrize("name", CASES)
def test_golden_cases_in_process(ctx, tmp_path, name):
    case = VEC['cases'][CASES.index(name)]
    db, indirs = M.write_case(str(tmp_path / 'in'), VEC, case)
    samples = mspecies.identify_samples(dict(indirs=indirs, max_samples=case['max_samples']))
    with mspecies.merge(ctx, samples, mspecies.read_species_ids(db), case['sample_depth']) as res:
        got = files_of(res, tmp_path / 'out', [s.id for s in samples])
        side = res.side_cells
    for f in M.FILES:
        assert got[f] == case['outputs'][f], f
    if name.startswith('hand'):
        assert side > 0           # 17 and more digits, 1e-320, ' 0.5 ', ' 9 ', 1_0: the host's parser


@pytest.mark.parametrize("name", CASES)
def test_golden_cases_through_the_script(tmp_path, name):
    case = VEC['cases'][CASES.index(name)]
    db, indirs = M.write_case(str(tmp_path / 'in'), VEC, case)
    out = str(tmp_path / 'out')
    argv = [out, '-i', ','.join(indirs), '-t', 'list', '-d', db, '--sample_depth', str(case['sample_depth']), '--profile']
    if case['max_samples'] is not None:
        argv += ['--max_samples', str(case['max_samples'])]
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'merge_species.py')] + argv, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stderr.replace(str(tmp_path / 'in') + os.sep, '') == case['stderr']
    for f in M.FILES:
        assert open(os.path.join(out, f)).read() == case['outputs'][f], f
    assert os.path.getsize(os.path.join(out, 'readme.txt')) > 0
    for phase in abi.SPECIES_MERGE_PHASES + ('write',):
        assert phase in r.stdout


@pytest.mark.parametrize("n", [1, 2, 3, 7, 8, 9, 10, 127, 128, 129, 130, 137, 257])
def test_rows_at_the_edges_of_the_pairwise_reduce(ctx, tmp_path, n):
    ids, sample_ids, profiles = M.synth(12, n, SEED + n)
    want = M.merge(sample_ids, profiles, ids, 1.0)
    with merged(ctx, tmp_path, ids, sample_ids, profiles) as res:
        assert res.lds_rows and res.lines == 13 * n
        same(res, want)
        assert files_of(res, tmp_path / 'out', sample_ids) == want['files']


@pytest.mark.parametrize("n", [130, 257])
def test_long_rows_equal_the_rows_sorted_in_lds(ctx, tmp_path, n):
    ids, sample_ids, profiles = M.synth(12, n, SEED + n)
    want = M.merge(sample_ids, profiles, ids, 1.0)
    with merged(ctx, tmp_path, ids, sample_ids, profiles) as lds, merged(ctx, tmp_path, ids, sample_ids, profiles, lds_bound=64) as long_rows:
        assert lds.lds_rows and not long_rows.lds_rows
        same(long_rows, want)
        for name in NAMES:
            assert bits(getattr(long_rows, name)) == bits(getattr(lds, name)) and bits(long_rows.rounded[name]) == bits(lds.rounded[name])
        assert long_rows.order.tolist() == lds.order.tolist()


def test_groups_of_files_change_nothing(ctx, tmp_path):
    ids, sample_ids, profiles = M.synth(12, 9, SEED)
    # sample 4 is larger than the small chunks: dropped lines in front of, between and behind its rows
    rows = profiles[4].split('\n')
    profiles[4] = '\n'.join(rows[:1] + ['a dropped line\t%d' % k for k in range(120)] + rows[1:7] + ['', 'x\ty\tz\tw\tv'] + rows[7:-1] + ['not\ta row']) + '\n'
    sizes = [len(p) + 1 for p in profiles]
    assert sizes[4] > 2 * max(sizes[:4] + sizes[5:])
    want = M.merge(sample_ids, profiles, ids, 1.0)
    with merged(ctx, tmp_path, ids, sample_ids, profiles) as one:
        assert one.groups == 1 and one.side_cells > 0
        same(one, want)
        base = files_of(one, tmp_path / 'out', sample_ids)
        assert base == want['files']
    for chunk, groups in ((max(sizes[:4] + sizes[5:]), 9), (16, 9), (sizes[0] + sizes[1] + sizes[2] + 8, None), (sum(sizes) - 1, 2)):
        with merged(ctx, tmp_path, ids, sample_ids, profiles, chunk_bytes=chunk) as res:
            assert res.groups == groups or (groups is None and 2 < res.groups < 9), (chunk, res.groups)
            assert res.lines == one.lines and res.side_cells == one.side_cells
            same(res, want)
            assert files_of(res, tmp_path / ('out_%d' % chunk), sample_ids) == base


def test_columns_rows_and_spellings_on_the_device(ctx, tmp_path):
    ids = ['a', 'bb', 'ccc']
    p0 = HEAD + 'a\t1\t1.5\t0.5\nbb\t2\t2.5\t0.25\nccc\t3\t0.0\t0.25\n'
    p1 = 'note\trelative_abundance\tspecies_id\tcoverage\tcoverage\tcount_reads\n' \
         'n\t 0.5 \tccc\t9\t1e-320\t1_0\n\nshort\tline\nn\t0.12345678901234567890\ta\t9\t123456789012345678\t 7 \nn\t1e22\tbb\t9\t1e-22\t-0\n'
    p2 = HEAD.rstrip('\n') + '\tmore\n' + 'bb\t+5\t.5\t5.\tm\nccc\t123456789012345678\t1E2\t1e+2\tm\na\t0\t-0.0\t0.1e1\tm\n' + 'bb\t5\t0.5\t5.0\n'
    want = M.merge(['s0', 's1', 's2'], [p0, p1, p2], ids, 1.0)
    assert want['coverage'][0][1] == 123456789012345678.0 and want['reads'][2][2] == 123456789012345678 and want['coverage'][2][1] == 1e-320
    for chunk in (0, 16):
        with merged(ctx, tmp_path, ids, ['s0', 's1', 's2'], [p0, p1, p2], chunk_bytes=chunk) as res:
            same(res, want)
            assert res.side_cells >= 6
            assert files_of(res, tmp_path / ('out_%d' % chunk), ['s0', 's1', 's2']) == want['files']


GOOD = HEAD + 'a\t1\t1.0\t0.5\nb\t2\t2.0\t0.25\nc\t3\t3.0\t0.25\n'
REFUSALS = [
    ('unknown', GOOD.replace('b\t2', 'q\t2'), "species 'q' is not in species_info.txt"),
    ('missing', GOOD.replace('c\t3\t3.0\t0.25\n', ''), "species 'c' of species_info.txt has no line"),
    ('twice', GOOD + 'a\t1\t1.0\t0.5\n', "species 'a' stands on an earlier line too"),
    ('header', GOOD.replace('coverage', 'depth'), "the header has no column 'coverage'"),
    ('cell_f', GOOD.replace('2.0', 'two'), "coverage of species 'b' is not a number"),
    ('cell_i', GOOD.replace('\t3\t', '\t3.5\t'), "count_reads of species 'c' is not a number"),
    ('nan', GOOD.replace('0.5', 'nan'), "relative_abundance of species 'a' is not finite"),
    ('inf', GOOD.replace('3.0', '1e999'), "coverage of species 'c' is not finite"),
    ('int64', GOOD.replace('\t2\t', '\t9223372036854775808\t'), "count_reads of species 'b' is beyond 64 bits"),
    ('empty', '', "the header has no column 'species_id'"),
]


@pytest.mark.parametrize("chunk", [0, 40])
@pytest.mark.parametrize("kind", [r[0] for r in REFUSALS])
def test_refusals_name_the_earliest_line(ctx, tmp_path, kind, chunk):
    _, text, message = [r for r in REFUSALS if r[0] == kind][0]
    ids = ['a', 'b', 'c']
    # a later sample is wrong too, on an earlier line and for another reason: the earlier sample is the one named
    profiles = [GOOD, GOOD, text, GOOD.replace('a\t1\t', 'z\t1\t'), GOOD]
    want = M.first_error(profiles, ids)
    assert want is not None and want.sample == 2
    sample_ids = ['s%d' % k for k in range(5)]
    with pytest.raises(abi.MidasSnpsError) as e:
        merged(ctx, tmp_path, ids, sample_ids, profiles, chunk_bytes=chunk)
    path = os.path.join(str(tmp_path), 's2', 'species', 'species_profile.txt')
    assert e.value.bad[:2] == (want.reason, 2)
    assert e.value.message.startswith(path) and message in e.value.message
    if want.reason != M.MISSING:
        assert e.value.bad[2] == want.line and '%s line %d: ' % (path, want.line) in e.value.message


def test_a_species_without_a_line_counts_behind_its_profile(ctx, tmp_path):
    ids = ['a', 'b', 'c']
    short = GOOD.replace('c\t3\t3.0\t0.25\n', '')
    for profiles, sample, reason in (([GOOD, short, GOOD.replace('two', '2.0').replace('2.0', 'two')], 1, M.MISSING),
                                     ([GOOD, GOOD.replace('2.0', 'two'), short], 1, M.CELL + 1),
                                     ([short.replace('1.0', 'x')], 0, M.CELL + 1)):
        want = M.first_error(profiles, ids)
        assert (want.reason, want.sample) == (reason, sample)
        for chunk in (0, 16):
            with pytest.raises(abi.MidasSnpsError) as e:
                merged(ctx, tmp_path, ids, ['s%d' % k for k in range(len(profiles))], profiles, chunk_bytes=chunk)
            assert e.value.bad[:2] == (reason, sample)


def test_script_reports_a_refusal(tmp_path):
    ids, sample_ids, profiles = M.synth(5, 3, SEED)
    profiles[1] = profiles[1].replace(ids[2] + '\t', 'Unheard_of\t')
    M.write_samples(str(tmp_path / 'in'), sample_ids, profiles)
    db = tmp_path / 'db'
    db.mkdir()
    (db / 'species_info.txt').write_text('species_id\trep_genome\n' + ''.join('%s\tG\n' % s for s in ids))
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'merge_species.py'), str(tmp_path / 'out'), '-i', str(tmp_path / 'in'), '-t', 'dir',
                        '-d', str(db)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    line = 1 + [x.split('\t')[0] for x in profiles[1].split('\n')].index('Unheard_of')
    assert r.returncode == 1
    assert "\nError: %s line %d: species 'Unheard_of' is not in species_info.txt\n" % (tmp_path / 'in' / sample_ids[1] / 'species' / 'species_profile.txt', line) in r.stderr


def test_600_species_40_samples_through_the_script(tmp_path):
    ids, sample_ids, profiles = M.synth(600, 40, SEED + 600)
    want = M.merge(sample_ids, profiles, ids, 1.0)
    M.write_samples(str(tmp_path / 'in'), sample_ids, profiles)
    db = tmp_path / 'db'
    db.mkdir()
    (db / 'species_info.txt').write_text('species_id\trep_genome\n' + ''.join('%s\tG%d\n' % (s, k) for k, s in enumerate(ids)))
    out = str(tmp_path / 'out')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'merge_species.py'), out, '-i', str(tmp_path / 'in'), '-t', 'dir', '-d', str(db)],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=dict(os.environ, MIDAS_SNPS_TRACE='1'))
    assert r.returncode == 0 and r.stderr == '', r.stderr
    assert 'lookup + scatter' in r.stdout
    for f in M.FILES:
        assert open(os.path.join(out, f)).read() == want['files'][f], f
    assert len(set(want['prevalence'])) > 5 and len(set(want['prevalence'])) < 41        # ties: the order is the stable one
