"""snp_trees.py without a GPU: the sequential model (tests/snp_trees_model.py) against additive trees it must recover exactly,
the tie rule on a star, the command through the model (trees.run_pipeline's make_context) against call_consensus.py's FASTA
compared column by column, the sample selection, and every exit with its message."""
import contextlib
import io
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from midas_amd import abi
from midas_amd.analyze import cli, consensus, synth, trees
from tests import analyze_model
from tests import snp_trees_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_SAMPLES = 7


@pytest.fixture(scope="module")
def species(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("trees") / "species_1")
    return d, synth.write_species_dir(d, n_sites=3000, n_samples=N_SAMPLES)['sample_ids']


def _run(indir, options, out, dist=None, make_context=M.ModelContext):
    argv = [indir] + list(options) + ['--out', out] + (['--dist', dist] if dist else [])
    args = cli.trees_arguments(argv)
    cli.check_trees_args(args)
    with contextlib.redirect_stdout(io.StringIO()):
        return trees.run_pipeline(args, make_context=make_context)


def _leaves(newick):
    return re.findall(r'[(,]([^(),:;]+):', newick)


@pytest.mark.parametrize("n", [3, 4, 5, 17, 64])
def test_the_model_recovers_additive_trees_exactly(n):
    rng = np.random.default_rng(100 + n)
    for _ in range(4):
        dist, splits = M.random_tree(n, rng)
        assert np.array_equal(dist, dist.T) and not dist.diagonal().any()
        tree = M.nj_tree(dist)
        assert tree['join'].shape == (n - 3, 2) and tree['len'].shape == (n - 3, 2)
        assert M.tree_splits(n, tree) == splits             # the topology as leaf bipartitions, and every length, exactly


def test_a_star_is_joined_by_the_tie_rule():
    for n in (4, 5, 9, 33):
        tree = M.nj_tree(M.star_matrix(n))
        assert [tuple(x) for x in tree['join'].tolist()] == M.star_joins(n)
        assert tree['last'].tolist() == [0, n - 2, n - 1]
        # the pendant branches are half the distance each; the inner ones have no length
        assert tree['len'][:, 1].tolist() == [0.25] * (n - 3) and tree['len'][0, 0] == 0.25 and not tree['len'][1:, 0].any()
        assert tree['last_len'].tolist() == [0.0, 0.25, 0.25]


def _fasta(path):
    lines = open(path).read().splitlines()
    return {h[1:].split('\t')[0]: s for h, s in zip(lines[0::2], lines[1::2])}


@pytest.mark.parametrize("options", [[], ['--site_prev', '0.9', '--site_depth', '4', '--site_maf', '0.01'], ['--max_sites', '500', '--site_ratio', '2.0']])
def test_the_command_through_the_model_agrees_with_call_consensus_letter_by_letter(species, tmp_path, options):
    indir, ids = species
    nwk, pairs, fa = str(tmp_path / 'tree.nwk'), str(tmp_path / 'pairs.txt'), str(tmp_path / 'seqs.fa')
    _run(indir, options, nwk, pairs)
    args = cli.consensus_arguments([indir] + options + ['--out', fa])
    cli.check_consensus_args(args)
    consensus.run_pipeline(args, make_context=analyze_model.ModelContext)
    seq = _fasta(fa)
    rows = ['\t'.join(trees.PAIRS_HEADER)]
    for i in range(N_SAMPLES):
        for j in range(i + 1, N_SAMPLES):
            a, b = seq[ids[i]], seq[ids[j]]
            shared = [(x, y) for x, y in zip(a, b) if x != '-' and y != '-']
            differ = sum(x != y for x, y in shared)
            assert len(shared) > 100
            rows.append('%s\t%s\t%d\t%d\t%r' % (ids[i], ids[j], len(shared), differ, differ / len(shared)))
    assert open(pairs).read() == '\n'.join(rows) + '\n'
    text = open(nwk).read()
    assert sorted(_leaves(text)) == sorted(ids) and text.endswith(');\n') and text.count('(') == N_SAMPLES - 2
    assert (text, open(pairs).read()) == M.expected_files([indir] + options)


def test_keep_and_exclude_samples_change_the_leaves(species, tmp_path):
    indir, ids = species
    nwk = str(tmp_path / 'tree.nwk')
    _run(indir, ['--exclude_samples', '%s,%s' % (ids[1], ids[4])], nwk)
    assert sorted(_leaves(open(nwk).read())) == sorted(set(ids) - {ids[1], ids[4]})
    keep = [ids[0], ids[2], ids[3], ids[6]]
    res = _run(indir, ['--keep_samples', ','.join(keep)], nwk)
    assert sorted(_leaves(open(nwk).read())) == sorted(keep) and res['both'].shape == (4, 4)
    _run(indir, ['--max_samples', '3'], nwk)
    assert sorted(_leaves(open(nwk).read())) == ids[:3] and open(nwk).read().count('(') == 1


def _rewrite(src, dst, old, new):
    os.makedirs(dst)
    for name in ('snps_summary.txt', 'snps_info.txt', 'snps_freq.txt', 'snps_depth.txt'):
        with open(os.path.join(src, name)) as f:
            text = f.read()
        with open(os.path.join(dst, name), 'w') as f:
            f.write(text.replace(old, new))


def test_every_exit_with_its_message(species, tmp_path):
    indir, ids = species
    nwk = str(tmp_path / 'tree.nwk')
    with pytest.raises(SystemExit) as e:
        _run(indir, ['--max_samples', '2'], nwk)
    assert e.value.code == "\nError: a tree needs at least 3 samples; 2 selected\n"
    for k, bad in enumerate(['sample 003', 'sample(003', 'sample:003', "sample'003", 'sample,003', 'sample;003', 'sample]003']):
        d = str(tmp_path / ('bad_%d' % k) / 'species_1')
        _rewrite(indir, d, ids[3], bad)
        with pytest.raises(SystemExit) as e:
            _run(d, [], nwk)
        assert e.value.code.startswith("\nError: the sample id '%s' contains whitespace or one of ()[]':;," % bad)
    # a sample without a read anywhere is kept at no site: it shares no site with anyone, the first such pair is named
    d = str(tmp_path / 'empty' / 'species_1')
    _rewrite(indir, d, '\0', '\0')
    M.zero_depth_column(d, 2)
    with pytest.raises(SystemExit) as e:
        _run(d, [], nwk)
    assert e.value.code.startswith("\nError: the samples %s and %s have no site called in both of them" % (ids[0], ids[2]))
    assert all(o in e.value.code for o in ('--site_prev', '--sample_depth', '--sample_cov'))
    _run(d, ['--exclude_samples', ids[2]], nwk)             # ... and without it the tree is there
    # more samples than the device holds pair matrices for
    with pytest.raises(SystemExit) as e:
        _run(indir, [], nwk, make_context=lambda: M.ModelContext(sample_limit=5))
    assert e.value.code.startswith("\nError: 7 samples selected, but the distance matrix of at most 5 samples fits the free device memory")
    # the checks of the command line, and the script itself before it touches a device
    with pytest.raises(SystemExit) as e:
        cli.check_trees_args(cli.trees_arguments([indir, '--site_depth', '0']))
    assert e.value.code == "\nError: --site_depth must be >=1\n"
    with pytest.raises(SystemExit) as e:
        cli.check_trees_args(cli.trees_arguments([indir, '--site_prev', '1.5']))
    assert e.value.code == "\nError: --site_prev must be between 0 and 1\n"
    script = os.path.join(ROOT, 'scripts', 'snp_trees.py')
    r = subprocess.run([sys.executable, script, str(tmp_path / 'nowhere')], capture_output=True, text=True)
    assert r.returncode != 0 and "does not exist" in r.stderr
    r = subprocess.run([sys.executable, script, '-h'], capture_output=True, text=True)
    assert r.returncode == 0 and '--dist' in r.stdout and '--exclude_samples' in r.stdout and '--group_rows' not in r.stdout


def test_the_new_symbols_are_declared_bound_and_built_without_contraction():
    from midas_amd import build
    lib = abi.load_library()
    header = open(os.path.join(ROOT, 'include', 'midas_snps.h')).read()
    for sym in ['midas_sites_consensus_pairs'] + abi.TREE_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % sym, header) and getattr(lib, sym).argtypes is not None
    assert 'midas_sites_consensus_pairs' in abi.SITES_SYMBOLS and abi.TREE_SYMBOLS == ['midas_nj_tree']
    assert 'nj_tree.hip' in build.SOURCES and '-ffp-contract=off' in build.SOURCE_FLAGS['nj_tree.hip']
    assert abi.format_repr_f64([0.1, -0.0, 1e-07, 0.3333333333333333]) == [repr(x) for x in (0.1, -0.0, 1e-07, 0.3333333333333333)]
