"""midas_sites_scan_classes and snp_pnps.py on the GPU box.  With one class the classed sums kernel must give what the existing
kernel gives, pi by bits; with 2 and 4 classes what the sequential model gives (tests/pnps_model.py) for class layouts that put
its 64-row steps on their borders: no live lane, all 64, a class that is absent, a class in the last partial step only.  Per
gene: a gene that comes back, a gene of one class, sites without a gene.  Chains whose sequential sum differs from the fused
and from the tree-reduced one must come out sequential.  Then the refusals and the command."""
import contextlib
import io
import os
import subprocess
import sys

import numpy as np
import pytest

from midas_amd import abi
from midas_amd.analyze import cli, diversity, pnps, synth
from tests import analyze_model as AM
from tests import pnps_model as M
from tests import site_cases as SC
from tests import test_pnps_host as H

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float('inf')


@pytest.fixture(scope="module")
def ctx():
    with abi.Context(0) as c:
        yield c


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# every SITES_SUMS mode of test_gpu_analyze.MODES
MODES = [
    dict(flags=abi.SITES_SUMS),
    dict(flags=abi.SITES_SUMS | abi.SITES_PER_GENE),
    dict(flags=abi.SITES_SUMS | abi.SITES_POOLED, site_prev=0.3),
    dict(flags=abi.SITES_SUMS | abi.SITES_POOLED | abi.SITES_PER_GENE | abi.SITES_WEIGHT, site_maf=0.01),
    dict(flags=abi.SITES_SUMS | abi.SITES_ROUND, allele_support=0.7, site_ratio=2.0),
    dict(flags=abi.SITES_SUMS | abi.SITES_POOLED | abi.SITES_PER_GENE | abi.SITES_ROUND, max_sites=3000),
]
GROUPS = ((0, 0), (1000, 0), (777, 100000))
BASE = dict(site_depth=2, site_ratio=INF, allele_support=0.5, site_prev=0.0, site_maf=0.0, snp_maf=0.01, max_sites=-1)


class Species:
    def __init__(self, tmp_path_factory, n_sites, seed):
        d = str(tmp_path_factory.mktemp("pnps_sp") / "species_1")
        synth.write_species_dir(d, n_sites, 13, seed=seed, n_genes=37, block=7000)
        self.t = abi.SitesTables(d)
        self.n = n_sites
        self.cols = np.array([c for c in range(13) if c % 5 != 3])
        self.mean = self.t.mean_coverage[self.cols]
        self.mask = (np.random.default_rng(5).random(n_sites) < 0.9).astype(np.uint8)

    def args(self):
        return self.t.freq_text, self.t.depth_text


@pytest.fixture(scope="module")
def big(tmp_path_factory):
    return Species(tmp_path_factory, 12000, 13)


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    """Tables of 1, 63, 64, 65 and 130 sites: less than a step, a step but one row, a step, a step and a row, two and a bit."""
    return {n: Species(tmp_path_factory, n, 100 + n) for n in (1, 63, 64, 65, 130)}


def _same_sums(got, exp, what):
    for k in ('n_kept', 'no_gene', 'n_sites'):
        assert got[k] == exp[k], (what, k, got[k], exp[k])
    for k in ('snps', 'sites', 'depth'):
        assert got[k].shape == exp[k].shape and np.array_equal(got[k], exp[k]), (what, k)
    assert got['pi'].shape == exp['pi'].shape and np.array_equal(_bits(got['pi']), _bits(exp['pi'])), (what, 'pi')


@pytest.mark.parametrize("k", range(len(MODES)))
def test_one_class_is_the_existing_kernel(ctx, big, small, k):
    for sp in [big] + list(small.values()):
        kw = dict(BASE, site_gene=sp.t.gene, n_genes=sp.t.n_genes)
        kw.update(MODES[k])
        if sp.n < 12000 and kw['max_sites'] >= 0:
            kw['max_sites'] = sp.n // 3
        for group_rows, chunk in (GROUPS if sp.n == 12000 else ((0, 0), (50, 0))):
            old = ctx.sites_scan(*sp.args(), sp.mask, sp.cols, sp.mean, group_rows=group_rows, chunk_bytes=chunk, **kw)
            for cls in (None, np.zeros(sp.n, np.uint8)):
                new = ctx.sites_scan_classes(*sp.args(), sp.mask, cls, 1, sp.cols, sp.mean, group_rows=group_rows, chunk_bytes=chunk, **kw)
                assert new['pi'].shape == (1,) + old['pi'].shape
                _same_sums(dict(new, **{q: new[q][0] for q in ('pi', 'snps', 'sites', 'depth')}), old, (sp.n, MODES[k], group_rows))
                assert new['groups'] == old['groups']
        if sp.n == 12000:
            assert old['groups'] > 1 and old['sites'].sum() > 1000


def layout(name, n, n_classes, mask):
    """-> site_class uint8 [n].  Rows outside the mask take any value, out of range included: only masked rows have a class."""
    rng = np.random.default_rng(n * 7 + n_classes)
    r = np.arange(n)
    if name == 'alternating':
        cls = r % n_classes
    elif name == 'blocks_of_64':
        cls = (r // 64) % n_classes
    elif name == 'one_absent':
        cls = rng.integers(0, n_classes - 1, n)
        cls[cls == n_classes - 2] = n_classes - 1           # class n_classes - 2 never appears
    elif name == 'last_partial_step':
        cls = rng.integers(0, n_classes - 1, n)
        cls[(n - 1) // 64 * 64:] = n_classes - 1            # the last class: in the last, partial, step alone
    else:
        cls = rng.integers(0, n_classes, n)
    cls = cls.astype(np.uint8)
    cls[mask == 0] = 200
    return cls


LAYOUTS = ['alternating', 'blocks_of_64', 'one_absent', 'last_partial_step', 'random']


def test_the_layouts_are_what_their_names_say():
    mask = np.ones(130, np.uint8)
    for nc in (2, 4):
        c = layout('one_absent', 130, nc, mask)
        assert nc - 2 not in set(c.tolist()) and nc - 1 in set(c.tolist())
        c = layout('last_partial_step', 130, nc, mask)
        assert np.all(c[128:] == nc - 1) and nc - 1 not in set(c[:128].tolist())
        c = layout('blocks_of_64', 130, nc, mask)
        assert np.all(c[:64] == 0) and np.all(c[64:128] == 1)
        assert sorted(set(layout('random', 130, nc, mask).tolist())) == list(range(nc))
    m = mask.copy()
    m[5] = 0
    assert layout('random', 130, 4, m)[5] == 200


SMALL_MODES = [
    dict(flags=abi.SITES_SUMS),
    dict(flags=abi.SITES_SUMS | abi.SITES_PER_GENE),
    dict(flags=abi.SITES_SUMS | abi.SITES_POOLED | abi.SITES_PER_GENE | abi.SITES_WEIGHT, site_prev=0.3),
    dict(flags=abi.SITES_SUMS | abi.SITES_ROUND, max_sites=40),
    dict(flags=abi.SITES_SUMS | abi.SITES_POOLED, max_sites=40),
]


@pytest.mark.parametrize("name", LAYOUTS)
@pytest.mark.parametrize("n_classes", [2, 4])
def test_classes_match_the_model_at_the_step_borders(ctx, small, name, n_classes):
    for n, sp in small.items():
        cls = layout(name, n, n_classes, sp.mask)
        for mode in SMALL_MODES:
            kw = dict(BASE, site_gene=sp.t.gene, n_genes=sp.t.n_genes)
            kw.update(mode)
            exp = M.sites_scan_classes(*sp.args(), sp.mask, cls, n_classes, sp.cols, sp.mean, **kw)
            for group_rows in (0, 50) if n == 130 else (0,):
                got = ctx.sites_scan_classes(*sp.args(), sp.mask, cls, n_classes, sp.cols, sp.mean, group_rows=group_rows, **kw)
                if kw['max_sites'] >= 0:        # (the model stops where the loop stops, the device reads whole groups)
                    got['n_sites'] = exp['n_sites']
                _same_sums(got, exp, (n, name, n_classes, mode, group_rows))
            if n == 130 and name in ('alternating', 'last_partial_step', 'random') and mode is SMALL_MODES[0]:
                assert np.all(exp['sites'].reshape(n_classes, -1).sum(axis=1) > 0)


BIG_CASES = [('random', 4, MODES[1]), ('blocks_of_64', 2, MODES[3]), ('alternating', 2, MODES[4])]


@pytest.mark.parametrize("name, n_classes, mode", BIG_CASES)
def test_classes_match_the_model_at_every_group_size(ctx, big, name, n_classes, mode):
    """12 000 sites: row groups split gene runs and 64-row steps, and the accumulators of every class carry across them."""
    sp = big
    cls = layout(name, sp.n, n_classes, sp.mask)
    kw = dict(BASE, site_gene=sp.t.gene, n_genes=sp.t.n_genes)
    kw.update(mode)
    exp = M.sites_scan_classes(*sp.args(), sp.mask, cls, n_classes, sp.cols, sp.mean, **kw)
    groups = []
    for group_rows, chunk in GROUPS:
        got = ctx.sites_scan_classes(*sp.args(), sp.mask, cls, n_classes, sp.cols, sp.mean, group_rows=group_rows, chunk_bytes=chunk, **kw)
        _same_sums(got, exp, (name, n_classes, group_rows))
        groups.append(got['groups'])
    assert groups[0] == 1 and groups[1] > 1 and groups[2] >= groups[1], groups
    assert np.all(exp['sites'].reshape(n_classes, -1).sum(axis=1) > 100)


def test_per_gene_runs(ctx, small):
    """Genes laid by hand over 130 sites: gene 0 comes back behind gene 1 and again behind gene 2, changes fall on lane 63 / lane 0
    of a step and inside one; gene 3 holds class 1 alone; gene 4 has no site; sites without a gene stand inside the mask."""
    sp = small[130]
    gene = np.full(130, -1, np.int32)
    gene[2:20], gene[20:40], gene[40:63], gene[63], gene[64:90], gene[90:100], gene[104:125], gene[125:130] = 0, 1, 0, 2, 0, 3, 1, 0
    mask = sp.mask.copy()
    mask[[0, 1, 63, 64, 100, 101, 129]] = 1
    for n_classes in (2, 4):
        cls = (np.arange(130) % n_classes).astype(np.uint8)
        cls[90:100] = 1
        for flags in (abi.SITES_SUMS | abi.SITES_PER_GENE, abi.SITES_SUMS | abi.SITES_PER_GENE | abi.SITES_POOLED):
            kw = dict(BASE, site_gene=gene, n_genes=5, flags=flags)
            exp = M.sites_scan_classes(*sp.args(), mask, cls, n_classes, sp.cols, sp.mean, **kw)
            union = ctx.sites_scan(*sp.args(), mask, sp.cols, sp.mean, **kw)
            assert exp['no_gene'] == union['no_gene'] >= 4                                 # counted once, whatever the class
            assert exp['sites'][1, :, 3].sum() > 0 and exp['sites'][0, :, 3].sum() == 0 and exp['sites'][:, :, 4].sum() == 0
            assert exp['sites'][0, :, 0].sum() > 0 and exp['sites'][:, :, 2].sum() > 0
            for group_rows in (0, 45, 64, 63):
                got = ctx.sites_scan_classes(*sp.args(), mask, cls, n_classes, sp.cols, sp.mean, group_rows=group_rows, **kw)
                _same_sums(got, exp, (n_classes, flags, group_rows))


def _tree_sum(terms):
    """What a wave would get by reducing its 64 lanes pairwise, steps of 64 added up in turn."""
    total = 0.0
    for k in range(0, len(terms), 64):
        v = list(terms[k:k + 64]) + [0.0] * (64 - len(terms[k:k + 64]))
        w = 32
        while w:
            v = [v[i] + v[i + w] for i in range(w)]
            w //= 2
        total += v[0]
    return total


def _order_tables():
    """Two chains of frequencies in one table, rows alternating: class 0 the rows of site_cases.fma_cases, class 1 a searched
    chain.  For both, sample 0's sequential pi differs in bits from the fused one (pi_chain); for the searched chain from the
    tree-reduced one too."""
    fma = SC.fma_cases()[0]
    chains = [[list(r) for r in fma.frows]]
    for seed in range(500, 700):
        rng = np.random.default_rng(seed)
        rows = [['%.17g' % x for x in rng.random(2)] for _ in range(len(fma.frows))]
        fs = [float(a) for a, _ in rows]
        terms = [(2.0 * f) * (1.0 - f) for f in fs]
        if SC.pi_chain(fs, False) != SC.pi_chain(fs, True) and SC.pi_chain(fs, False) != _tree_sum(terms):
            chains.append(rows)
            break
    assert len(chains) == 2
    frows, drows, cls = [], [], []
    for r in range(len(fma.frows)):
        for c in (0, 1):
            frows.append(chains[c][r])
            drows.append(fma.drows[r])
            cls.append(c)
    return chains, frows, drows, np.array(cls, np.uint8)


def test_the_order_tables_are_what_they_claim():
    chains, frows, _, cls = _order_tables()
    for c in (0, 1):
        fs = [float(a) for a, _ in chains[c]]
        assert [r[0] for r, k in zip(frows, cls) if k == c] == [a for a, _ in chains[c]]
        seq = SC.pi_chain(fs, False)
        assert seq != SC.pi_chain(fs, True)
        if c == 1:
            assert seq != _tree_sum([(2.0 * f) * (1.0 - f) for f in fs])


def test_pi_is_the_sequential_sum_of_every_class(ctx):
    chains, frows, drows, cls = _order_tables()
    n = len(frows)
    freq, depth = SC.matrix(frows), SC.matrix(drows)
    for flags in (abi.SITES_SUMS, abi.SITES_SUMS | abi.SITES_POOLED):
        kw = dict(site_depth=1, site_ratio=INF, allele_support=0.0, site_prev=0.0, site_maf=0.0, flags=flags)
        exp = M.sites_scan_classes(freq, depth, np.ones(n, np.uint8), cls, 2, [0, 1], [10.0, 10.0], **kw)
        if flags == abi.SITES_SUMS:
            for c in (0, 1):
                assert exp['pi'][c, 0, 0] == SC.pi_chain([float(a) for a, _ in chains[c]], False)
        for group_rows in (0, 7):
            got = ctx.sites_scan_classes(freq, depth, np.ones(n, np.uint8), cls, 2, [0, 1], [10.0, 10.0], group_rows=group_rows, **kw)
            _same_sums(got, exp, (flags, group_rows))


def test_refusals_leave_the_context_usable(ctx, small):
    sp = small[65]
    kw = dict(BASE, flags=abi.SITES_SUMS)
    ok = np.zeros(65, np.uint8)
    bad = ok.copy()
    row = int(np.flatnonzero(sp.mask)[3])
    bad[row] = 2
    for cls, n_classes, flags in ((bad, 2, abi.SITES_SUMS), (ok, 0, abi.SITES_SUMS), (ok, 5, abi.SITES_SUMS), (ok, 2, abi.SITES_SUMS | abi.SITES_SEQ),
                                  (ok, 2, abi.SITES_SEQ), (None, 2, abi.SITES_SUMS)):
        with pytest.raises(abi.MidasSnpsError) as e:
            ctx.sites_scan_classes(*sp.args(), sp.mask, cls, n_classes, sp.cols, sp.mean, **dict(kw, flags=flags, minor=ok, major=ok))
        assert e.value.status == abi.ERR_INVALID_ARG, (n_classes, flags)
    # an unmasked row may hold any class
    off = sp.mask.copy()
    off[row] = 0
    exp = M.sites_scan_classes(*sp.args(), off, bad, 2, sp.cols, sp.mean, **kw)
    _same_sums(ctx.sites_scan_classes(*sp.args(), off, bad, 2, sp.cols, sp.mean, **kw), exp, 'after the refusals')


# ---- the command ---------------------------------------------------------------------------------------------------------------------
class _Shared:
    """The module's context, handed to run_pipeline: its close() leaves the context to the fixture."""

    def __init__(self, ctx):
        self._ctx = ctx

    def sites_scan(self, *a, **kw):
        return self._ctx.sites_scan(*a, **kw)

    def sites_scan_classes(self, *a, **kw):
        return self._ctx.sites_scan_classes(*a, **kw)

    def close(self):
        pass


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return H.write_tree(str(tmp_path_factory.mktemp("pnps_gpu")))


@pytest.mark.parametrize("k", range(len(H.CASES)))
def test_snp_pnps_on_the_device_writes_the_references_blocks(ctx, tree, tmp_path, k):
    H.check_case(tree, H.CASES[k], str(tmp_path / 'pnps.txt'), make_context=lambda: _Shared(ctx))


def test_the_script_itself_against_the_golden(tree, tmp_path):
    case = [c for c in H.CASES if c['species'] == 'small' and 'per-gene' in c['options'] and 'pooled-samples' in c['options'] and c['seed'] is None][0]
    out = str(tmp_path / 'out.txt')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'snp_pnps.py')] + H.argv_of(tree, case, out) + ['--group_rows', '17'],
                       capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr + r.stdout
    got = open(out).read()
    for name in pnps.CLASSES:
        assert H.sorted_rows(H.project(got, name), True) == H.sorted_rows(case['out_' + name], True)
    H.check_ratio(got)
    assert "Script: snp_pnps.py" in r.stdout and "pN/pS options:" in r.stdout


@pytest.mark.parametrize("opts", [['--genomic_type', 'per-gene', '--rand_sites', '0.7', '--seed', '5', '--site_depth', '3'],
                                  ['--sample_type', 'pooled-samples', '--weight_by_depth', '--site_prev', '0.5', '--group_rows', '1000']])
def test_the_blocks_are_two_snp_diversity_runs_on_the_device(ctx, big, tmp_path, opts):
    d = big.t.dir
    out = str(tmp_path / 'pnps.txt')
    with contextlib.redirect_stdout(io.StringIO()):
        args = cli.pnps_arguments([d, '--out', out] + opts)
        cli.check_pnps_args(args)
        pnps.run_pipeline(args, make_context=lambda: _Shared(ctx))
        got = open(out).read()
        for name in pnps.CLASSES:
            one = str(tmp_path / ('pi_%s.txt' % name))
            a = cli.diversity_arguments([d, '--out', one, '--locus_type', 'CDS', '--site_type', name] + opts)
            cli.check_diversity_args(a)
            diversity.run_pipeline(a, make_context=lambda: _Shared(ctx))
            assert H.project(got, name) == open(one).read(), name
    n_na, n = H.check_ratio(got)
    assert n_na < n and len(got.splitlines()) == n + 1 >= 2
