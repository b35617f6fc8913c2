"""strain_tracking.py on the GPU box: midas_sites_id_markers and midas_sites_track_markers against the sequential model
(tests/strains_model.py), every integer, at several group sizes and at sample counts around the pair kernel's tile; both
commands against the reference's own output (tests/golden/strain_vectors.json), in process and through the script; and the
chain merge_midas.py snps -> id_markers -> track_markers."""
import os
import subprocess
import sys

import numpy as np
import pytest

from midas_amd import abi
from midas_amd import synth as reads_synth
from midas_amd.analyze import strains, synth
from tests import strains_model as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VEC = M.load_vectors()
GROUPS = ((0, 0), (777, 100000), (50, 0))          # one group; not a multiple of 64; fewer rows than a word of the bit matrix


@pytest.fixture(scope="module")
def ctx():
    with abi.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return M.write_tree(str(tmp_path_factory.mktemp("strains_gpu")), VEC)


def _species(tmp_path_factory, n_sites, n_samples, seed, **kw):
    d = str(tmp_path_factory.mktemp("sp") / "species_1")
    synth.write_strain_species_dir(d, n_sites, n_samples, seed=seed, block=7000, **kw)
    return abi.SitesTables(d)


def _which(t, rows, n):
    """The per-site byte of track_markers for the marker rows of id_markers."""
    minor = strains.allele_codes(t, 'minor_allele', n)
    which = np.zeros(n, np.uint8)
    which[rows[:, 0]] = np.where(rows[:, 1] == minor[rows[:, 0]], 2, 1)
    return which


def _upper(both):
    return np.triu(both)


def test_device_calls_match_the_sequential_model_at_every_group_size(ctx, tmp_path_factory):
    n_sites, n_samples = 9000, 13
    t = _species(tmp_path_factory, n_sites, n_samples, seed=13)
    cols = np.array([c for c in range(n_samples) if c != 4])
    mi, ma = strains.allele_codes(t, 'minor_allele', n_sites), strains.allele_codes(t, 'major_allele', n_sites)
    for kw in (dict(min_freq=0.1, min_reads=3, allele_prev=1), dict(min_freq=0.3, min_reads=6, allele_prev=3)):
        exp = M.sites_id_markers(t.freq_text, t.depth_text, mi, ma, cols, **kw)
        assert len(exp['rows']) > 500
        which = _which(t, exp['rows'], n_sites)
        exp_t = M.sites_track_markers(t.freq_text, t.depth_text, which, cols, kw['min_freq'], kw['min_reads'])
        assert exp_t['n_matched'] == len(exp['rows']) and not np.triu(exp_t['both'], 1).all()
        assert np.triu(exp_t['both'], 1).any() == (kw['allele_prev'] > 1)       # a private allele is shared by no pair
        groups = []
        for group_rows, chunk in GROUPS:
            got = ctx.sites_id_markers(t.freq_text, t.depth_text, mi, ma, cols, group_rows=group_rows, chunk_bytes=chunk, **kw)
            assert np.array_equal(got['rows'], exp['rows']), (kw, group_rows)
            assert got['n_sites'] == n_sites and got['side_freq'] == 0 and got['side_depth'] == 0
            got_t = ctx.sites_track_markers(t.freq_text, t.depth_text, which, cols, kw['min_freq'], kw['min_reads'], group_rows=group_rows,
                                            chunk_bytes=chunk)
            assert np.array_equal(_upper(got_t['both']), exp_t['both']), (kw, group_rows)
            assert got_t['n_matched'] == exp_t['n_matched'] and got_t['n_sites'] == n_sites
            groups.append((got['groups'], got_t['groups']))
        assert groups[0] == (1, 1) and groups[1][0] > 1 and groups[2][0] > groups[1][0] and groups[2][1] == groups[2][0], groups
    # rows called and rows read: the row behind the last one called is still checked
    got = ctx.sites_id_markers(t.freq_text, t.depth_text, mi[:4000], ma[:4000], cols, 0.1, 3, 1, n_parse=4001, group_rows=777)
    exp = M.sites_id_markers(t.freq_text, t.depth_text, mi[:4000], ma[:4000], cols, 0.1, 3, 1, n_parse=4001)
    assert np.array_equal(got['rows'], exp['rows']) and got['n_sites'] == 4001


def test_pair_kernel_over_several_word_runs_and_staging_steps(ctx, tmp_path_factory):
    """One row group with thousands of matched sites: the pair kernel's words are cut into several runs (workgroups along
    blockIdx.y that add to the same accumulator cells), a run takes several staging steps of 32 words, and the last run ends
    in the middle of a step.  pair_blocks sets how many workgroups the cut aims at; the sums must not depend on it."""
    n_sites, n_samples = 40000, 13
    t = _species(tmp_path_factory, n_sites, n_samples, seed=40, private=0.45, shared=0.3, common=0.05)
    cols = np.arange(n_samples)
    mi, ma = strains.allele_codes(t, 'minor_allele', n_sites), strains.allele_codes(t, 'major_allele', n_sites)
    rows = M.sites_id_markers(t.freq_text, t.depth_text, mi, ma, cols, 0.1, 3, 4)['rows']
    which = _which(t, rows, n_sites)
    exp = M.sites_track_markers(t.freq_text, t.depth_text, which, cols, 0.1, 3)
    step = 64 * 32                                    # matched sites a staging step holds
    assert exp['n_matched'] > 8 * step and np.triu(exp['both'], 1).any()
    n_words = (exp['n_matched'] + 63) // 64
    assert n_words % 32 != 0                          # the last run's last step is a partial one
    shapes = set()
    for pair_blocks, group_rows in ((0, 0), (4, 0), (3, 0), (1, 0), (2, 30011)):
        got = ctx.sites_track_markers(t.freq_text, t.depth_text, which, cols, 0.1, 3, group_rows=group_rows, pair_blocks=pair_blocks)
        assert np.array_equal(_upper(got['both']), exp['both']), (pair_blocks, group_rows)
        assert got['n_matched'] == exp['n_matched'] and got['groups'] == (1 if group_rows == 0 else 2)
        shapes.add((got['pair_runs'], got['pair_steps']))
        if pair_blocks == 0:
            assert got['pair_runs'] == (n_words + 31) // 32 > 8 and got['pair_steps'] == 1
        elif pair_blocks > 1:
            assert got['pair_runs'] == pair_blocks and got['pair_steps'] >= 2
            if group_rows == 0:                       # the runs are whole steps, so the last run is the short one
                assert n_words % (32 * got['pair_steps']) != 0
        else:
            assert got['pair_runs'] == 1 and got['pair_steps'] == (n_words + 31) // 32 > 8
    assert len(shapes) == 5


def test_the_error_in_the_earlier_row_is_reported_at_every_group_size(ctx):
    S, N = 4, 40
    matrix = lambda rows: np.frombuffer(''.join('%d\t%s\n' % (r + 1, '\t'.join(row)) for r, row in enumerate(rows)).encode(), np.uint8)
    for call_row, cell_row in ((10, 30), (30, 10), (12, 12)):
        frows = [['0.5'] * S for _ in range(N)]
        drows = [['7'] * S for _ in range(N)]
        drows[cell_row][1] = 'x'
        minor, major = np.zeros(N, np.uint8), np.ones(N, np.uint8)
        minor[call_row] = 255
        frows[call_row][3] = 'inf' if call_row != cell_row else '0.5'
        which = np.full(N, 2, np.uint8)
        for group_rows in (0, 64, 7):
            first_call = call_row < cell_row
            with pytest.raises(abi.MidasSnpsError) as e:
                ctx.sites_id_markers(matrix(frows), matrix(drows), minor, major, np.arange(S), 0.1, 3, 1, group_rows=group_rows)
            assert e.value.bad == ((4, call_row, 0) if first_call else (2, cell_row, 1)), (call_row, cell_row, group_rows)
            with pytest.raises(abi.MidasSnpsError) as e:
                ctx.sites_track_markers(matrix(frows), matrix(drows), which, np.arange(S), 0.1, 3, group_rows=group_rows)
            assert e.value.bad == ((3, call_row, 3) if first_call else (2, cell_row, 1)), (call_row, cell_row, group_rows)


@pytest.mark.parametrize("n", [1, 2, abi.SITES_PAIR_TILE - 1, abi.SITES_PAIR_TILE + 1, 150])
def test_sample_counts_around_the_pair_tile(ctx, tmp_path_factory, n):
    n_sites = 2500
    t = _species(tmp_path_factory, n_sites, 150, seed=150)
    cols = np.arange(150)[::-1][:n].copy() if n > 2 else np.arange(n)
    mi, ma = strains.allele_codes(t, 'minor_allele', n_sites), strains.allele_codes(t, 'major_allele', n_sites)
    exp = M.sites_id_markers(t.freq_text, t.depth_text, mi, ma, cols, 0.1, 3, 2)
    # every planted site is a marker site here, whatever these samples make of it: the bit matrix has columns no sample sets
    rows = M.sites_id_markers(t.freq_text, t.depth_text, mi, ma, np.arange(150), 0.1, 3, 4)['rows']
    which = _which(t, rows, n_sites)
    exp_t = M.sites_track_markers(t.freq_text, t.depth_text, which, cols, 0.1, 3)
    assert exp_t['n_matched'] > 300 and exp_t['both'].trace() > 0
    for group_rows, chunk in GROUPS[:2]:
        got = ctx.sites_id_markers(t.freq_text, t.depth_text, mi, ma, cols, 0.1, 3, 2, group_rows=group_rows, chunk_bytes=chunk)
        assert np.array_equal(got['rows'], exp['rows']), group_rows
        got_t = ctx.sites_track_markers(t.freq_text, t.depth_text, which, cols, 0.1, 3, group_rows=group_rows, chunk_bytes=chunk)
        assert np.array_equal(_upper(got_t['both']), exp_t['both']), group_rows
        assert got_t['n_matched'] == exp_t['n_matched']
        assert got_t['word_pairs'] >= n * (n + 1) // 2 * ((exp_t['n_matched'] + 63) // 64)


@pytest.mark.parametrize("freq, depth, which_bad", [("0.5x", "5", (1, 3, 2)), ("0.5", "abc", (2, 3, 2)), ("inf", "5", (3, 3, 2))])
def test_rows_that_cannot_be_read_or_called_are_reported_with_their_place(ctx, freq, depth, which_bad):
    S, N = 4, 6
    matrix = lambda rows: np.frombuffer(''.join('%d\t%s\n' % (r + 1, '\t'.join(row)) for r, row in enumerate(rows)).encode(), np.uint8)
    frows = [['0.5'] * S for _ in range(N)]
    drows = [['7'] * S for _ in range(N)]
    frows[3][2], drows[3][2] = freq, depth
    codes = np.zeros(N, np.uint8), np.ones(N, np.uint8)
    with pytest.raises(abi.MidasSnpsError) as e:
        ctx.sites_id_markers(matrix(frows), matrix(drows), *codes, np.arange(S), 0.1, 3, 1)
    assert e.value.bad == which_bad
    with pytest.raises(abi.MidasSnpsError) as e:
        ctx.sites_track_markers(matrix(frows), matrix(drows), np.full(N, 2, np.uint8), np.arange(S), 0.1, 3)
    assert e.value.bad == which_bad
    # a letter that is none of the four, where a sample has the allele
    frows[3][2], drows[3][2] = '0.5', '7'
    codes[0][4] = 255
    with pytest.raises(abi.MidasSnpsError) as e:
        ctx.sites_id_markers(matrix(frows), matrix(drows), *codes, np.arange(S), 0.1, 3, 1)
    assert e.value.bad == (4, 4, 0)
    res = ctx.sites_id_markers(matrix(frows), matrix(drows), codes[0][:4], codes[1][:4], np.arange(S), 0.1, 3, 1, n_parse=5)
    assert res['n_sites'] == 5 and len(res['rows']) == 0          # both letters in all four samples: no marker


class _Shared:
    """The module's context, handed to the hosts: its close() leaves the context to the fixture."""

    def __init__(self, ctx):
        self._ctx = ctx

    def sites_id_markers(self, *a, **kw):
        return self._ctx.sites_id_markers(*a, **kw)

    def sites_track_markers(self, *a, **kw):
        return self._ctx.sites_track_markers(*a, **kw)

    def close(self):
        pass


@pytest.mark.parametrize("k", range(len(VEC['id_markers'])))
def test_id_markers_on_the_device_writes_the_references_bytes(ctx, tree, tmp_path, k):
    M.check_case(tree, 'id_markers', VEC['id_markers'][k], str(tmp_path / 'markers.txt'), make_context=lambda: _Shared(ctx), marker_names=VEC['markers'])


@pytest.mark.parametrize("k", range(len(VEC['track_markers'])))
def test_track_markers_on_the_device_writes_the_references_bytes(ctx, tree, tmp_path, k):
    M.check_case(tree, 'track_markers', VEC['track_markers'][k], str(tmp_path / 'sharing.txt'), make_context=lambda: _Shared(ctx), marker_names=VEC['markers'])


def _script(*argv):
    return subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'strain_tracking.py')] + list(argv), capture_output=True, text=True, cwd=ROOT)


def test_the_script_itself_against_the_golden(tree, tmp_path):
    """The real command line, each run in its own process, at a group size that cuts the species into many groups."""
    for program, cases in (('id_markers', VEC['id_markers'][:3] + VEC['id_markers'][6:7]), ('track_markers', VEC['track_markers'][1:4] + VEC['track_markers'][6:])):
        for case in cases:
            out = str(tmp_path / 'out.txt')
            r = _script(*M.argv_of(tree, program, case, out, VEC['markers']), '--group_rows', '17')
            assert r.returncode == 0, r.stderr + r.stdout
            with open(out, newline='') as f:
                assert f.read() == M.expected_out(case)
            assert r.stdout.endswith(case['printed']) and "MIDAS: Metagenomic Intra-species Diversity Analysis System" in r.stdout


def test_merge_midas_snps_then_id_markers_then_track_markers(tmp_path):
    """The chain: this project's own merge writes the tables; the two commands' outputs are the sequential model's."""
    data = reads_synth.make_merge_dataset(str(tmp_path / "samples"), n_samples=5, n_sites=6000, seed=11)
    merged = str(tmp_path / "merged")
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'merge_midas.py'), 'snps', merged, '-i', os.path.dirname(data['samples'][0]),
                        '-t', 'dir', '-d', data['db'], '--all_sites'], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr + r.stdout
    d = os.path.join(merged, 'sp1')
    assert abi.SitesTables(d).n_sites > 1000
    for opts in (['--allele_prev', '1'], ['--allele_prev', '2', '--min_reads', '2']):
        markers, exp = str(tmp_path / 'markers.txt'), str(tmp_path / 'markers_model.txt')
        r = _script('id_markers', '--indir', d, '--out', markers, *opts)
        assert r.returncode == 0, r.stderr + r.stdout
        M.run(merged, 'id_markers', dict(species='sp1', options=opts), exp)
        assert open(markers).read() == open(exp).read()
        sharing, exp = str(tmp_path / 'sharing.txt'), str(tmp_path / 'sharing_model.txt')
        r = _script('track_markers', '--indir', d, '--markers', markers, '--out', sharing)
        assert r.returncode == 0, r.stderr + r.stdout
        M.run(merged, 'track_markers', dict(species='sp1', options=['--markers', markers]), exp)
        assert open(sharing).read() == open(exp).read() and len(open(sharing).read().splitlines()) == 1 + 10
    assert len(open(markers).read().splitlines()) > 1
