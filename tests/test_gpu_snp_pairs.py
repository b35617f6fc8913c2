"""midas_sites_pair_diversity and snp_pairs.py on the GPU box.  All seven arrays of the device call must equal the sequential
model (tests/pairs_model.py), the doubles by bits: at the borders of the staging run (16 rows), of the wave's 64 rows and of
both tile sides (16 and 64 samples), for both kernel forms and every row grouping, on chains whose sequential sum differs from
the fused and from the tree-reduced one, and on hand-written rows that sit on each decision.  Then the cross-checks against the
existing device paths, the refusals and the script."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from midas_amd import abi
from midas_amd.analyze import synth
from tests import pairs_model as M
from tests import site_cases as SC
from tests import test_gpu_pnps as P
from tests import test_snp_pairs_host as H

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float('inf')
BASE = dict(site_depth=2, site_ratio=INF, allele_support=0.5, site_prev=0.0, site_maf=0.0, snp_maf=0.01, max_sites=-1, flags=0)
RUN = 16                    # sites_pairs.hip kSpRun: rows staged at a time
FORMS = (1, 2)              # one pair a lane (tiles of 16 x 16), a 4 x 4 patch a lane (tiles of 64 x 64)


@pytest.fixture(scope="module")
def ctx():
    with abi.Context(0) as c:
        yield c


def same(got, exp, what, any_nan=False):
    """any_nan: where both hold a NaN, its sign and payload are not compared (IEEE 754 leaves them open; every other double,
    the infinities included, still by bits)."""
    for k in M.KEYS_INT:
        assert np.array_equal(got[k], exp[k]), (what, k)
    for k in M.KEYS_F64:
        g, e = H.bits(got[k]), H.bits(exp[k])
        if any_nan:
            both = np.isnan(got[k]) & np.isnan(exp[k])
            g, e = np.where(both, 0, g), np.where(both, 0, e)
        assert np.array_equal(g, e), (what, k)
    assert got['n_sites'] == exp['n_sites'] and got['n_masked'] == exp['n_masked'], what


def modes(n_sites):
    """Five option sets: plain, weighted, rounded, site_prev 0.5, max_sites at a third of the sites (with site_prev 1.0 the pairs
    retain different rows, so each fills it at a row of its own)."""
    return [dict(), dict(flags=abi.SITES_WEIGHT, site_prev=0.5), dict(flags=abi.SITES_ROUND, site_maf=0.05),
            dict(site_prev=0.5, site_maf=0.01, allele_support=0.7, site_ratio=2.0), dict(max_sites=n_sites // 3, site_prev=1.0)]


class Wide:
    """n_sites x 75 columns; a case selects some of them, not in a row."""

    def __init__(self, tmp_path_factory, n_sites):
        d = str(tmp_path_factory.mktemp("pairs_sp") / "species_1")
        synth.write_species_dir(d, n_sites, 75, seed=300 + n_sites)
        self.t = abi.SitesTables(d)
        self.n = n_sites
        self.mask = (np.random.default_rng(n_sites).random(n_sites) < 0.9).astype(np.uint8)
        self.mask[-1] = 1

    def pick(self, S):
        cols = np.array([c for c in range(75) if c % 15 != 4][:S])
        return cols, self.t.mean_coverage[cols]

    def args(self):
        return self.t.freq_text, self.t.depth_text


SITE_COUNTS = (1, RUN - 1, RUN, RUN + 1, 63, 64, 65, 130)


@pytest.fixture(scope="module")
def wide(tmp_path_factory):
    return {n: Wide(tmp_path_factory, n) for n in SITE_COUNTS}


BORDERS = [(n, S) for n in SITE_COUNTS for S in (2, 3, 17)] + [(130, S) for S in (15, 16, 63, 64, 65, 70)]


@pytest.mark.parametrize("n_sites, S", BORDERS)
def test_borders_of_runs_and_tiles(ctx, wide, n_sites, S):
    sp = wide[n_sites]
    cols, mean = sp.pick(S)
    for mode in modes(n_sites):
        kw = dict(BASE)
        kw.update(mode)
        exp = M.sites_pair_diversity(*sp.args(), sp.mask, cols, mean, **kw)
        for form in FORMS:
            got = ctx.sites_pair_diversity(*sp.args(), sp.mask, cols, mean, pair_form=form, **kw)
            same(got, exp, (n_sites, S, mode, form))
            assert got['pair_form'] == (1, 4)[form - 1] and got['tiles'] == (lambda s: s * (s + 1) // 2)(-(-S // (16, 64)[form - 1]))
    if n_sites == 130:
        assert exp['sites'][0, 1] <= 130 // 3 and exp['shared'][np.triu_indices(S, 1)].sum() > 0


@pytest.fixture(scope="module")
def big(tmp_path_factory):
    return P.Species(tmp_path_factory, 12000, 13)


BIG_MODES = [dict(site_prev=0.5, max_sites=3000), dict(flags=abi.SITES_WEIGHT | abi.SITES_ROUND, site_maf=0.01)]


@pytest.mark.parametrize("mode", BIG_MODES)
def test_both_forms_at_every_group_size(ctx, big, mode):
    """12 000 sites: the accumulators of every pair carry across the row groups, whichever form folds them."""
    kw = dict(BASE)
    kw.update(mode)
    exp = M.sites_pair_diversity(*big.args(), big.mask, big.cols, big.mean, **kw)
    for form in FORMS:
        groups = []
        for group_rows, chunk in P.GROUPS:
            got = ctx.sites_pair_diversity(*big.args(), big.mask, big.cols, big.mean, group_rows=group_rows, chunk_bytes=chunk, pair_form=form, **kw)
            same(got, exp, (mode, form, group_rows))
            groups.append(got['groups'])
        assert groups[0] == 1 and groups[1] > 1 and groups[2] >= groups[1], groups
    assert exp['shared'][np.triu_indices(len(big.cols), 1)].min() > 100
    if kw['max_sites'] >= 0:
        assert exp['sites'].max() == kw['max_sites']
    # the form chosen for so few samples is the first
    assert ctx.sites_pair_diversity(*big.args(), big.mask, big.cols, big.mean, **kw)['pair_form'] == 1


def test_many_samples_in_small_groups(ctx, tmp_path_factory):
    sp = Wide(tmp_path_factory, 300)
    cols, mean = sp.pick(70)
    kw = dict(BASE, site_prev=0.5)
    exp = M.sites_pair_diversity(*sp.args(), sp.mask, cols, mean, **kw)
    for form in FORMS:
        for group_rows in (0, 50, 63, 64):
            same(ctx.sites_pair_diversity(*sp.args(), sp.mask, cols, mean, group_rows=group_rows, pair_form=form, **kw), exp, (form, group_rows))


# ---- the order of the adds ----------------------------------------------------------------------------------------------------------
def _sums(rows, contract):
    """pi, w1 and x of a two-sample table as written, or with every product fused into the addition that takes it."""
    pi = w1 = x = 0.0
    for a, b in rows:
        p = ((0.0 + a) + b) / 2
        if contract:
            pi = SC.fused(2.0 * p, 1.0 - p, pi)
            w1 = SC.fused(2.0 * a, 1.0 - a, w1)
            x = SC.fused(b, 1.0 - a, SC.fused(a, 1.0 - b, 0.0)) + x
        else:
            pi += (2.0 * p) * (1.0 - p)
            w1 += (2.0 * a) * (1.0 - a)
            x += (a * (1.0 - b)) + (b * (1.0 - a))
    return pi, w1, x


def _terms(rows):
    ps = [((0.0 + a) + b) / 2 for a, b in rows]
    return [(2.0 * p) * (1.0 - p) for p in ps], [(2.0 * a) * (1.0 - a) for a, _ in rows], [(a * (1.0 - b)) + (b * (1.0 - a)) for a, b in rows]


def order_table():
    """The rows of site_cases.fma_cases followed by a searched chain: pi, w1 and x of the whole table each differ in bits between
    the sequential, the fused and the tree-reduced sum."""
    head = [list(r) for r in SC.fma_cases()[0].frows]
    for seed in range(900, 1400):
        rng = np.random.default_rng(seed)
        frows = head + [['%.17g' % v for v in rng.random(2)] for _ in range(90)]
        rows = [(float(a), float(b)) for a, b in frows]
        seq, fus = _sums(rows, False), _sums(rows, True)
        tree = [P._tree_sum(t) for t in _terms(rows)]
        if all(seq[k] != fus[k] and seq[k] != tree[k] for k in range(3)):
            return frows, rows
    raise AssertionError('order_table')


def test_the_order_table_is_what_it_claims():
    _, rows = order_table()
    seq, fus, tree = _sums(rows, False), _sums(rows, True), [P._tree_sum(t) for t in _terms(rows)]
    assert all(seq[k] != fus[k] and seq[k] != tree[k] for k in range(3)) and len(rows) == 130


def test_the_sums_are_sequential(ctx):
    frows, rows = order_table()
    n = len(frows)
    freq, depth = SC.matrix(frows), SC.matrix([['5', '7']] * n)
    kw = dict(BASE, allele_support=0.0)
    exp = M.sites_pair_diversity(freq, depth, np.ones(n, np.uint8), [0, 1], [10.0, 10.0], **kw)
    seq = _sums(rows, False)
    assert (exp['pi'][0, 1], exp['w1'][0, 1], exp['x'][0, 1]) == seq and exp['shared'][0, 1] == n
    for form in FORMS:
        for group_rows in (0, 7):
            same(ctx.sites_pair_diversity(freq, depth, np.ones(n, np.uint8), [0, 1], [10.0, 10.0], group_rows=group_rows, pair_form=form, **kw),
                 exp, (form, group_rows))


# ---- every decision at its border ---------------------------------------------------------------------------------------------------
def _run_rows(ctx, frows, drows, mean=None, any_nan=False, **opts):
    """-> (model, rows every pair retained) after the device gave the model's arrays in both forms."""
    n, S = len(frows), len(frows[0])
    freq, depth = SC.matrix(frows), SC.matrix(drows)
    kw = dict(BASE)
    kw.update(opts)
    mean = [10.0] * S if mean is None else mean
    rows = {}
    exp = M.sites_pair_diversity(freq, depth, np.ones(n, np.uint8), list(range(S)), mean, _rows_out=rows, **kw)
    for form in FORMS:
        same(ctx.sites_pair_diversity(freq, depth, np.ones(n, np.uint8), list(range(S)), mean, pair_form=form, **kw), exp, (opts, form), any_nan)
    return exp, rows


def test_decisions_at_their_borders(ctx):
    # one cell of the two kept: prevalence 0.5 is on --site_prev 0.5 and below 0.500001
    f, d = [['0.2', '0.3', '0.1']] * 3, [['5', '0', '5'], ['5', '5', '5'], ['0', '0', '5']]
    _, rows = _run_rows(ctx, f, d, site_prev=0.5)
    assert rows[(0, 1)] == [0, 1] and rows[(0, 2)] == [0, 1, 2] and rows[(1, 2)] == [0, 1, 2]
    _, rows = _run_rows(ctx, f, d, site_prev=0.500001)
    assert rows[(0, 1)] == [1] and rows[(0, 2)] == [0, 1] and rows[(1, 2)] == [1]
    # allele_support: max(f, 1 - f) on the value and to either side of it (site_cases.support_cases)
    cells = ['0.55', '0.54999999999999993', '0.5500000000000002', '0.45', '0.44999999999999996', '0.45000000000000007']
    exp, _ = _run_rows(ctx, [[c, '0.9'] for c in cells], [['5', '5']] * len(cells), allele_support=0.55)
    assert exp['shared'][0, 1] == 4 and exp['sites'][0, 1] == len(cells)
    # site_maf: the pooled frequency of 0.2 and 0.3 is 0.25 itself
    f = [['0.2', '0.3'], ['0.2', '0.29999999999999993'], ['0.2', '0.3000000000000002']]
    assert ((0.0 + 0.2) + 0.3) / 2 == 0.25 and ((0.0 + 0.2) + 0.29999999999999993) / 2 < 0.25 < ((0.0 + 0.2) + 0.3000000000000002) / 2
    _, rows = _run_rows(ctx, f, [['5', '5']] * 3, site_maf=0.25, allele_support=0.0)
    assert rows[(0, 1)] == [0, 2]
    _, rows = _run_rows(ctx, f, [['5', '9']] * 3, site_maf=SC.up(0.25), allele_support=0.0)
    assert rows[(0, 1)] == [2]
    # snp_maf: min(p, 1 - p) on 0.01 from either end, and just off it
    f = [['0.01', '0.01'], ['0.99', '0.99'], ['0.009999999999999998', '0.009999999999999998'], ['0.9900000000000001', '0.9900000000000001']]
    exp, _ = _run_rows(ctx, f, [['5', '5']] * 4, snp_maf=0.01)
    assert exp['snps'][0, 1] == 2 and exp['sites'][0, 1] == 4
    # --weight_by_depth: depths that make the two cells count 1 : 1000
    _run_rows(ctx, [['0.1', '0.7', '0.3'], ['0.123456789', '0.3', '0.9']], [['2', '2000', '999999999999'], ['3', '100000000000000000', '7']],
              flags=abi.SITES_WEIGHT, allele_support=0.0)


# Without --consensus nan and inf are frequencies like any other: the sums carry them.  A sum that holds a NaN must hold one on
# the device too, but which sign the NaN has is not compared: IEEE 754 leaves it open, and 1.0 - nan keeps the sign on a CPU where
# the device's subtraction (an addition of the negated operand) flips it.  Beside inf stand frequencies above 1, so that no sum
# forms inf - inf or inf x 0: the sums of the inf rows are infinities, compared by bits.
NAN_ROWS = [['0.1', '0.2', '0.3'], ['0.2', 'nan', '0.4'], ['0.3', '0.1', '0.2']]
INF_ROWS = [['0.1', '0.2', '0.3'], ['inf', '1.5', '2.5'], ['0.3', '0.1', '0.2']]


def test_nan_and_inf_are_numbers_until_they_are_rounded(ctx):
    d = [['5', '5', '5']] * 3
    exp, _ = _run_rows(ctx, NAN_ROWS, d, any_nan=True, allele_support=0.0)
    assert np.isnan(exp['pi'][0, 1]) and np.isnan(exp['x'][1, 2]) and np.isfinite(exp['pi'][0, 2]) and exp['sites'][0, 1] == 3
    exp, _ = _run_rows(ctx, INF_ROWS, d, allele_support=0.0)
    assert exp['pi'][0, 1] == -INF and exp['x'][0, 2] == -INF and np.isfinite(exp['pi'][1, 2])
    for frows, sample in ((NAN_ROWS, 1), (INF_ROWS, 0)):
        n = len(frows)
        for opts in (dict(), dict(max_sites=1), dict(group_rows=1)):
            args = (SC.matrix(frows), SC.matrix(d), np.ones(n, np.uint8), [0, 1, 2], [10.0] * 3)
            kw = dict(BASE, flags=abi.SITES_ROUND, **opts)
            with pytest.raises(abi.MidasSnpsError) as model:
                M.sites_pair_diversity(*args, **kw)
            with pytest.raises(abi.MidasSnpsError) as e:
                ctx.sites_pair_diversity(*args, **kw)
            assert e.value.status == abi.ERR_BAD_LAYOUT and e.value.bad == model.value.bad == (3, 1, sample), (opts, e.value.bad)


# ---- against the existing device paths -------------------------------------------------------------------------------------------------
class _Shared:
    """The module's context, handed to run_pipeline: its close() leaves the context to the fixture."""

    def __init__(self, ctx):
        self._ctx = ctx

    def __getattr__(self, name):
        return getattr(self._ctx, name)

    def close(self):
        pass


@pytest.mark.parametrize("opts", [['--site_prev', '0.5', '--group_rows', '1000'], ['--weight_by_depth', '--site_maf', '0.01', '--max_sites', '2000']])
def test_rows_are_snp_diversity_runs_on_the_device(ctx, big, tmp_path, opts):
    d = big.t.dir
    ids = big.t.strings('sample_id')
    text, _, _ = H.run_pairs([d, '--out', str(tmp_path / 'pairs.txt')] + opts, make_context=lambda: _Shared(ctx))
    got = H.project(text)
    assert len(got) == 78
    for a, b in ((ids[0], ids[1]), (ids[3], ids[11]), (ids[7], ids[12])):
        assert got[(a, b)] == H.separate_run(d, a, b, opts, str(tmp_path / 'pi.txt'), make_context=lambda: _Shared(ctx)), (a, b)


def test_rounded_pairs_are_the_consensus_pairs(ctx, big):
    """Under --consensus, without a site filter: a site shared by a pair is a site called in both samples, and a (1 - b) + b (1 - a)
    of two rounded frequencies is 1 where the calls differ.  rint and `>= 0.5` part ways on a frequency of 0.5 itself: such rows
    are masked out of both calls."""
    rows = np.array([[float(c) for c in r[1:]] for r in M.M._rows(big.t.freq_text)])[:, big.cols]
    half = (rows == 0.5).any(axis=1)
    assert half.sum() <= 0.05 * big.n
    mask = big.mask & ~half
    new = ctx.sites_pair_diversity(*big.args(), mask, big.cols, big.mean, **dict(BASE, flags=abi.SITES_ROUND))
    old = ctx.sites_consensus_pairs(*big.args(), mask, big.cols, big.mean, 2, INF, 0.5, 0.0, 0.0)
    up = np.triu_indices(len(big.cols), 1)
    assert np.array_equal(new['shared'][up], old['both'][up]) and np.array_equal(new['x'][up], old['diff'][up].astype(np.float64))
    assert old['diff'][up].min() > 0


# ---- refusals and the script ---------------------------------------------------------------------------------------------------------
def _raw_call(ctx, sp, cols, mean, null=None):
    """The C call itself, with one output pointer null."""
    import ctypes as C
    ft, dt = np.ascontiguousarray(sp.t.freq_text), np.ascontiguousarray(sp.t.depth_text)
    S = len(cols)
    c32, m64 = np.ascontiguousarray(cols, np.int32), np.ascontiguousarray(mean, np.float64)
    fp, ip = np.array([INF, 0.5, 0.0, 0.0, 0.01]), np.array([2, -1, 0, 0, 0, 0, 0, 0], np.int64)
    outs = [np.zeros((S, S), np.int64) for _ in range(3)] + [np.zeros((S, S), np.float64) for _ in range(4)]
    stats, ms = np.zeros(16, np.int64), np.zeros(8, np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    return ctx._lib.midas_sites_pair_diversity(ctx._h, p(ft), ft.shape[0], p(dt), dt.shape[0], sp.n, p(sp.mask), S, p(c32), p(m64), p(fp), p(ip),
                                               *[None if k == null else p(a) for k, a in enumerate(outs)], p(stats), p(ms))


def test_refusals_leave_the_context_usable(ctx, wide):
    sp = wide[65]
    cols, mean = sp.pick(3)
    for bad in (dict(cols=cols[:1], mean=mean[:1]), dict(group_rows=-1), dict(chunk_bytes=-1), dict(pair_form=-1), dict(pair_form=3),
                dict(flags=abi.SITES_WEIGHT, site_depth=0)):
        kw = dict(BASE)
        kw.update({k: v for k, v in bad.items() if k not in ('cols', 'mean')})
        with pytest.raises(abi.MidasSnpsError) as e:
            ctx.sites_pair_diversity(*sp.args(), sp.mask, bad.get('cols', cols), bad.get('mean', mean), **kw)
        assert e.value.status == abi.ERR_INVALID_ARG, bad
    for null in range(7):
        assert _raw_call(ctx, sp, cols, mean, null) == abi.ERR_INVALID_ARG
    assert _raw_call(ctx, sp, cols, mean) == 0
    same(ctx.sites_pair_diversity(*sp.args(), sp.mask, cols, mean, **BASE), M.sites_pair_diversity(*sp.args(), sp.mask, cols, mean, **BASE),
         'after the refusals')


def test_the_script_itself(tmp_path):
    d = str(tmp_path / 'species_1')
    ids = H.write_species(d)
    opts = ['--site_prev', '0.5', '--snp_maf', '0.05']
    exp_table, exp_tree = H.expected_table([d, '--out', str(tmp_path / 'exp.txt'), '--tree', str(tmp_path / 'exp.nwk')] + opts)
    out, nwk = str(tmp_path / 'pairs.txt'), str(tmp_path / 'da.nwk')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'snp_pairs.py'), d, '--out', out, '--tree', nwk, '--group_rows', '17'] + opts,
                       capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr + r.stdout
    assert open(out).read() == exp_table and open(nwk).read() == exp_tree
    assert sorted(re.findall(r'sample_\d+', open(nwk).read())) == sorted(ids)
    assert "Script: snp_pairs.py" in r.stdout and "Pair options:" in r.stdout
