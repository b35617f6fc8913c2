"""snp_trees.py on the GPU box: midas_sites_consensus_pairs against the sequential model (tests/snp_trees_model.py), every
integer, at sample counts past one and two borders of the pair kernel's tile, at several group sizes and word-run cuts;
midas_nj_tree against the model, joins equal and lengths bit for bit, on matrices full of ties, on a star and on additive trees
it must recover exactly; the script in its own process; and the chain merge_midas.py snps -> snp_trees.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

from midas_amd import abi
from midas_amd import synth as reads_synth
from midas_amd.analyze import sites, synth
from tests import snp_trees_model as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_SITES, N_COLUMNS = 2600, 135
DROPPED, ZERO = (4, 70, 101), 9              # matrix columns no sample reads; the column without a read


@pytest.fixture(scope="module")
def ctx():
    with abi.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def wide(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("trees_wide") / "species_1")
    synth.write_species_dir(d, N_SITES, N_COLUMNS, seed=21, block=1000)
    M.zero_depth_column(d, ZERO)
    return abi.SitesTables(d)


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("trees_small") / "species_1")
    synth.write_species_dir(d, n_sites=3000, n_samples=7)
    return d


@pytest.mark.parametrize("S", [65, 130])
def test_consensus_pairs_match_the_model_at_every_group_size_and_run_cut(ctx, wide, S):
    cols = [c for c in range(N_COLUMNS) if c not in DROPPED][:S]
    assert len(cols) == S and ZERO in cols and cols != list(range(S))
    mean = wide.mean_coverage[cols]
    mask = sites.info_mask(wide)
    opts = dict(site_depth=3, site_ratio=3.0, allele_support=0.5, site_prev=0.8, site_maf=0.0)
    exp = M.sites_consensus_pairs(wide.freq_text, wide.depth_text, mask, cols, mean, **opts)
    step = 64 * 32
    assert step < exp['n_kept'] < N_SITES and exp['n_kept'] % 64 != 0          # past a staging run of the planes, a partial last word
    z = cols.index(ZERO)
    assert not exp['both'][z].any() and not exp['both'][:, z].any() and exp['diff'].any()
    assert np.triu(exp['both'], 1)[np.arange(S) != z][:, np.arange(S) != z].max() > 1000
    seen = set()
    for group_rows, pair_blocks in ((0, 0), (0, 1), (1000, 0), (777, 2)):
        got = ctx.sites_consensus_pairs(wide.freq_text, wide.depth_text, mask, cols, mean, group_rows=group_rows, pair_blocks=pair_blocks, **opts)
        assert np.array_equal(got['both'], exp['both']), (group_rows, pair_blocks)
        assert np.array_equal(got['diff'], exp['diff']), (group_rows, pair_blocks)
        assert got['n_kept'] == exp['n_kept'] and got['n_sites'] == N_SITES and got['side_freq'] == 0 and got['side_depth'] == 0
        assert got['groups'] == (1 if group_rows == 0 else -(-N_SITES // group_rows)) and got['sample_limit'] > S
        seen.add((got['groups'], got['pair_runs'], got['pair_steps']))
    assert len(seen) == 4 and (1, 1, -(-exp['n_kept'] // 64 // 16)) in seen      # one run of every staging step; several runs
    if S > 65:
        return
    # --max_sites ends the walk in the middle of a group; a --site_list mask stands alone
    for kw in (dict(max_sites=700), dict(flags=abi.SITES_MASK_ONLY)):
        exp = M.sites_consensus_pairs(wide.freq_text, wide.depth_text, mask, cols, mean, **opts, **kw)
        got = ctx.sites_consensus_pairs(wide.freq_text, wide.depth_text, mask, cols, mean, group_rows=500, **opts, **kw)
        assert np.array_equal(got['both'], exp['both']) and np.array_equal(got['diff'], exp['diff']) and got['n_kept'] == exp['n_kept']
    assert got['n_kept'] == N_SITES


def _same_tree(got, exp):
    assert np.array_equal(got['join'], exp['join']) and np.array_equal(got['last'], exp['last'])
    assert got['len'].tobytes() == exp['len'].tobytes() and got['last_len'].tobytes() == exp['last_len'].tobytes()


@pytest.mark.parametrize("n", [3, 4, 5, 63, 64, 65, 257])
def test_nj_tree_matches_the_model_bit_for_bit_on_matrices_full_of_ties(ctx, n):
    rng = np.random.default_rng(n)
    negative = 0
    for most in (6, 3):
        d = M.ratio_matrix(n, rng, most)
        exp = M.nj_tree(d)
        _same_tree(ctx.nj_tree(d), exp)
        negative += int((exp['len'] < 0).sum())
        if n > 5:
            assert np.unique(d).shape[0] < n            # far fewer values than pairs: equal distances everywhere
    assert negative > 0 or n < 63


@pytest.mark.parametrize("n", [4, 5, 9, 33, 130])
def test_nj_tree_joins_a_star_by_the_tie_rule(ctx, n):
    got = ctx.nj_tree(M.star_matrix(n))
    assert [tuple(x) for x in got['join'].tolist()] == M.star_joins(n) and got['last'].tolist() == [0, n - 2, n - 1]
    _same_tree(got, M.nj_tree(M.star_matrix(n)))


@pytest.mark.parametrize("n", [3, 4, 5, 17, 64])
def test_nj_tree_recovers_additive_trees_exactly(ctx, n):
    rng = np.random.default_rng(100 + n)
    for _ in range(4):
        dist, splits = M.random_tree(n, rng)
        got = ctx.nj_tree(dist)
        assert M.tree_splits(n, got) == splits
        _same_tree(got, M.nj_tree(dist))


def test_nj_tree_refuses_what_is_no_distance_matrix(ctx):
    d = M.star_matrix(5)
    d[1, 3] = d[3, 1] = float('nan')
    with pytest.raises(abi.MidasSnpsError):
        ctx.nj_tree(d)


def _script(*argv):
    return subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'snp_trees.py')] + list(argv), capture_output=True, text=True, cwd=ROOT)


def test_the_script_itself_writes_the_models_files(small, tmp_path):
    nwk, pairs = str(tmp_path / 'tree.nwk'), str(tmp_path / 'pairs.txt')
    options = ['--site_prev', '0.8', '--site_depth', '3', '--exclude_samples', 'sample_005']
    r = _script(small, '--out', nwk, '--dist', pairs, '--group_rows', '17', *options)
    assert r.returncode == 0, r.stderr + r.stdout
    assert "MIDAS: Metagenomic Intra-species Diversity Analysis System" in r.stdout and "Script: snp_trees.py" in r.stdout
    exp = M.expected_files([small] + options)
    assert open(nwk).read() == exp[0] and open(pairs).read() == exp[1]
    assert exp[0].count('sample_') == 6 and len(exp[1].splitlines()) == 1 + 15


def test_merge_midas_snps_then_snp_trees(tmp_path):
    """The chain: this project's own merge writes the tables, and the tree and the distances are the sequential model's."""
    data = reads_synth.make_merge_dataset(str(tmp_path / "samples"), n_samples=5, n_sites=6000, seed=11)
    merged = str(tmp_path / "merged")
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'merge_midas.py'), 'snps', merged, '-i', os.path.dirname(data['samples'][0]),
                        '-t', 'dir', '-d', data['db'], '--all_sites'], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr + r.stdout
    d = os.path.join(merged, 'sp1')
    assert abi.SitesTables(d).n_sites > 1000
    nwk, pairs = str(tmp_path / 'tree.nwk'), str(tmp_path / 'pairs.txt')
    for options in ([], ['--site_maf', '0.05', '--site_depth', '3']):
        r = _script(d, '--out', nwk, '--dist', pairs, *options)
        assert r.returncode == 0, r.stderr + r.stdout
        exp = M.expected_files([d] + options)
        assert open(nwk).read() == exp[0] and open(pairs).read() == exp[1]
        assert len(exp[1].splitlines()) == 1 + 10 and exp[0].count('(') == 3
        assert any(int(row.split('\t')[3]) > 0 for row in exp[1].splitlines()[1:])
