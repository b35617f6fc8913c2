"""snp_ld.py on the GPU box: midas_sites_ld against the sequential model (tests/snp_ld_model.py), the integer counts exactly and
the three sums bit for bit, at sample counts around the borders of a 64-sample word, over positions laid out around the retained
sites (runs longer than a 64-partner step, gaps of exactly the window and one more, three contigs), at several group sizes and
anchor chunks; --within gene, --min_samples at its border, --max_sites, a mask that stands alone, a malformed cell; the script in
its own process; and the chain merge_midas.py snps -> snp_ld.py."""
import contextlib
import io
import os
import subprocess
import sys

import numpy as np
import pytest

from midas_amd import abi
from midas_amd import synth as reads_synth
from midas_amd.analyze import cli, ld, sites, synth
from tests import snp_ld_model as M
from tests import snp_trees_model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_SITES, N_COLUMNS = 2600, 135
DROPPED, ZERO = (4, 70, 101), 9              # matrix columns no sample reads; the column without a read
MAX_DIST, BIN_WIDTH = 150, 20                # eight bins, the last one 141-150
OPTS = dict(site_depth=3, site_ratio=3.0, allele_support=0.5, site_prev=0.7, site_maf=0.0)
SUMS = ('sum_r2', 'sum_d2', 'sum_het')


@pytest.fixture(scope="module")
def ctx():
    with abi.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def wide(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("ld_wide") / "species_1")
    synth.write_species_dir(d, N_SITES, N_COLUMNS, seed=21, block=1000)
    snp_trees_model.zero_depth_column(d, ZERO)
    return abi.SitesTables(d)


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("ld_small") / "species_1")
    synth.write_species_dir(d, n_sites=3000, n_samples=7)
    ref_id, ref_pos = M.spread_positions(3000, np.arange(3000), 100, seed=3)
    locus, gene = M.gene_runs(3000)
    M.rewrite_info(d, dict(ref_id=ref_id, ref_pos=ref_pos, locus_type=locus, gene_id=gene))
    return d


def _columns(S):
    cols = [c for c in range(N_COLUMNS) if c not in DROPPED][:S]
    if ZERO not in cols:
        cols = sorted(cols[:-1] + [ZERO])
    assert len(cols) == S and ZERO in cols
    return cols


_CASES = {}


def _case(wide, S):
    """The inputs of one sample count and the model's result, computed once: the columns, the mask, the keys laid out around the
    sites these options retain, the genes."""
    if S not in _CASES:
        cols = _columns(S)
        mean = wide.mean_coverage[cols]
        mask = sites.info_mask(wide)
        mask[::11] = False
        rows = M.consensus_calls(wide.freq_text, wide.depth_text, mask, cols, mean, **OPTS)['rows']
        ref_id, ref_pos = M.spread_positions(N_SITES, rows, MAX_DIST, seed=S)
        contig = np.unique(ref_id, return_inverse=True)[1].astype(np.int64)           # (the names sort in order of appearance)
        key = contig * (1 << 40) + np.array(ref_pos, np.int64)
        gene = np.array([int(g[5:]) if g else -1 for g in M.gene_runs(N_SITES)[1]], np.int32)
        base = dict(freq_text=wide.freq_text, depth_text=wide.depth_text, site_mask=mask, sample_col=cols, mean_depth=mean, site_key=key, site_gene=gene)
        exp = M.sites_ld(max_dist=MAX_DIST, bin_width=BIN_WIDTH, **base, **OPTS)
        _CASES[S] = (base, exp)
    return _CASES[S]


def _same(got, exp, what=None, stopped=False):
    """stopped: --max_sites ended the walk; the device then counts the rows of the groups it took up, as the sibling entries do."""
    assert np.array_equal(got['window'], exp['window']) and np.array_equal(got['pairs'], exp['pairs']), what
    for k in SUMS:
        assert got[k].dtype == np.float64 and got[k].tobytes() == exp[k].tobytes(), (what, k)
    assert (got['n_kept'], got['pairs_visited']) == (exp['n_kept'], exp['pairs_visited']), what
    assert exp['n_sites'] <= got['n_sites'] <= N_SITES and (stopped or got['n_sites'] == exp['n_sites']), what


@pytest.mark.parametrize("S", [7, 64, 65, 130])
def test_ld_matches_the_model_at_every_group_size_and_anchor_chunk(ctx, wide, S):
    base, exp = _case(wide, S)
    key = exp['key']
    M_ = exp['n_kept']
    assert M.means_something(exp) and 1000 < M_ < N_SITES - 200 and MAX_DIST % BIN_WIDTH != 0
    # an anchor with more than one 64-partner step and a partial last one; neighbours exactly the window and one more apart;
    # pairs at both ends of a bin; three contigs, one of a single retained site; the last site has partners before it and none after
    partners = np.searchsorted(key, key + MAX_DIST, side='right') - np.arange(M_) - 1
    assert partners.max() > 64 and partners.max() % 64 != 0 and partners[-1] == 0 and partners[-2] == 1
    step = np.diff(key)
    assert (step == MAX_DIST).sum() >= 1 and (step == MAX_DIST + 1).sum() >= 1
    assert all(np.isin(key + d, key).any() for d in (BIN_WIDTH, BIN_WIDTH + 1, 3 * BIN_WIDTH, 3 * BIN_WIDTH + 1, MAX_DIST))
    assert np.bincount(key >> 40).tolist()[1] == 1 and np.bincount(key >> 40).shape[0] == 3 and exp['window'][-1] > 0
    seen = set()
    for group_rows in (0, 1000, 777):
        for anchor_chunk in (0, 1, 100):
            got = ctx.sites_ld(max_dist=MAX_DIST, bin_width=BIN_WIDTH, group_rows=group_rows, anchor_chunk=anchor_chunk, **base, **OPTS)
            _same(got, exp, (group_rows, anchor_chunk))
            assert got['side_freq'] == 0 and got['side_depth'] == 0 and got['site_limit'] > N_SITES
            assert got['groups'] == (1 if group_rows == 0 else -(-N_SITES // group_rows))
            assert got['anchor_chunks'] == (1 if anchor_chunk == 0 else -(-M_ // anchor_chunk))
            seen.add((got['groups'], got['anchor_chunks']))
    assert len(seen) == 9


def test_within_gene_pairs_only_the_sites_of_one_gene(ctx, wide):
    base, everywhere = _case(wide, 65)
    kw = dict(max_dist=MAX_DIST, bin_width=BIN_WIDTH, flags=abi.SITES_LD_SAME_GENE, **base, **OPTS)
    exp = M.sites_ld(**kw)
    gene = base['site_gene'][exp['rows']]
    assert M.means_something(exp) and (gene < 0).sum() > 100 and np.unique(gene).shape[0] > 30
    assert 0 < exp['window'].sum() < everywhere['window'].sum() and (exp['window'] <= everywhere['window']).all()
    for group_rows, anchor_chunk in ((0, 0), (777, 100)):
        _same(ctx.sites_ld(group_rows=group_rows, anchor_chunk=anchor_chunk, **kw), exp, (group_rows, anchor_chunk))
    # without the flag the genes are not looked at, and need not be there
    _same(ctx.sites_ld(max_dist=MAX_DIST, bin_width=BIN_WIDTH, **dict(base, site_gene=None), **OPTS), everywhere)


def test_min_samples_at_its_border(ctx, wide):
    """A pair with n samples called at both sites counts under --min_samples n and not under n + 1."""
    base, exp = _case(wide, 7)
    hist = exp['n_hist']
    N = max(n for n in hist if n - 1 in hist)
    assert hist[N] > 0 and hist[N - 1] > 0 and N >= 3
    res = {}
    for n in (N - 1, N, N + 1):
        kw = dict(max_dist=MAX_DIST, bin_width=BIN_WIDTH, min_samples=n, **base, **OPTS)
        res[n] = M.sites_ld(**kw)
        _same(ctx.sites_ld(**kw), res[n], n)
    assert res[N - 1]['pairs'].sum() - res[N]['pairs'].sum() == hist[N - 1] and res[N]['pairs'].sum() - res[N + 1]['pairs'].sum() == hist[N]
    assert np.array_equal(res[N]['window'], res[N - 1]['window']) and M.means_something(res[N - 1])


def test_max_sites_inside_a_group_and_a_mask_that_stands_alone(ctx, wide):
    base, _ = _case(wide, 65)
    for kw in (dict(max_sites=0), dict(max_sites=700), dict(flags=abi.SITES_MASK_ONLY)):
        kw = dict(max_dist=MAX_DIST, bin_width=BIN_WIDTH, **base, **OPTS, **kw)
        exp = M.sites_ld(**kw)
        _same(ctx.sites_ld(group_rows=500, anchor_chunk=300, **kw), exp, kw.get('max_sites'), stopped='max_sites' in kw)
        if kw.get('max_sites') == 0:
            assert exp['n_kept'] == 0 and not exp['window'].any()
            continue
        assert M.means_something(exp)
    assert exp['n_kept'] == int(base['site_mask'].sum()) and M.sites_ld(**dict(kw, flags=0))['n_kept'] < exp['n_kept']
    got = ctx.sites_ld(group_rows=500, **dict(kw, max_sites=700, flags=0))
    rows = M.sites_ld(**dict(kw, max_sites=700, flags=0))['n_sites']
    assert got['n_kept'] == 700 and 700 < rows < N_SITES and rows % 500 not in (0, 1) and got['groups'] == -(-rows // 500) < -(-N_SITES // 500)


def test_a_malformed_cell_is_reported_where_consensus_pairs_reports_it(ctx, wide):
    base, _ = _case(wide, 65)
    text = np.array(wide.depth_text)
    ends = np.flatnonzero(text == ord('\n'))
    row = 1503
    tab = ends[row - 1] + 1 + int(np.flatnonzero(text[ends[row - 1] + 1:ends[row]] == ord('\t'))[2])
    text[tab + 1] = ord('x')                                                  # matrix column 2 of data row 1503
    bad = []
    common = dict(site_mask=base['site_mask'], sample_col=base['sample_col'], mean_depth=base['mean_depth'], **OPTS)
    for name, call in (('pairs', lambda: ctx.sites_consensus_pairs(wide.freq_text, text, group_rows=1000, **common)),
                       ('ld', lambda: ctx.sites_ld(wide.freq_text, text, site_key=base['site_key'], site_gene=None, group_rows=777, **common)),
                       ('model', lambda: M.sites_ld(wide.freq_text, text, site_key=base['site_key'], site_gene=None, **common))):
        with pytest.raises(abi.MidasSnpsError) as e:
            call()
        bad.append(e.value.bad)
    assert bad[0] == bad[1] == bad[2] == (2, row, base['sample_col'].index(2))
    # behind the row that fills --max_sites it is never read, though it lies in the group that was parsed
    kw = dict(site_key=base['site_key'], site_gene=None, max_sites=900, max_dist=MAX_DIST, bin_width=BIN_WIDTH, **common)
    exp = M.sites_ld(wide.freq_text, text, **kw)
    _same(ctx.sites_ld(wide.freq_text, text, **kw), exp, stopped=True)
    assert exp['n_kept'] == 900 and exp['n_sites'] < row


def _script(*argv):
    return subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'snp_ld.py')] + list(argv), capture_output=True, text=True, cwd=ROOT)


@pytest.mark.parametrize("options", [['--max_dist', '100', '--bin_width', '8', '--site_prev', '0.8', '--site_depth', '3', '--exclude_samples', 'sample_005'],
                                     ['--max_dist', '90', '--bin_width', '15', '--within', 'gene', '--min_samples', '5']])
def test_the_script_itself_writes_the_models_file(small, tmp_path, options):
    out, double = str(tmp_path / 'ld.txt'), str(tmp_path / 'double.txt')
    r = _script(small, '--out', out, '--group_rows', '170', '--anchor_chunk', '333', *options)
    assert r.returncode == 0, r.stderr + r.stdout
    assert "MIDAS: Metagenomic Intra-species Diversity Analysis System" in r.stdout and "Script: snp_ld.py" in r.stdout
    args = cli.ld_arguments([small, '--out', double] + options)
    cli.check_ld_args(args)
    with contextlib.redirect_stdout(io.StringIO()):
        exp = ld.run_pipeline(args, make_context=M.ModelContext)
    assert open(out).read() == open(double).read() == M.expected_file([small] + options)[0]
    assert M.means_something(exp) and len(open(out).read().splitlines()) == 1 + -(-args['max_dist'] // args['bin_width'])


def test_merge_midas_snps_then_snp_ld(tmp_path):
    """The chain: this project's own merge writes the tables, positions included, and the table is the sequential model's."""
    data = reads_synth.make_merge_dataset(str(tmp_path / "samples"), n_samples=5, n_sites=6000, seed=11)
    merged = str(tmp_path / "merged")
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'merge_midas.py'), 'snps', merged, '-i', os.path.dirname(data['samples'][0]),
                        '-t', 'dir', '-d', data['db'], '--all_sites'], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr + r.stdout
    d = os.path.join(merged, 'sp1')
    t = abi.SitesTables(d)
    assert t.n_sites > 1000 and len(t.contig_names) == 3
    out = str(tmp_path / 'ld.txt')
    for options in (['--bin_width', '100'], ['--max_dist', '300', '--bin_width', '25', '--min_samples', '3', '--site_depth', '3', '--site_maf', '0.01']):
        r = _script(d, '--out', out, *options)
        assert r.returncode == 0, r.stderr + r.stdout
        text, exp = M.expected_file([d] + options)
        assert open(out).read() == text
        assert M.means_something(exp) and 'NA' not in text
