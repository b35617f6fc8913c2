"""snp_diversity.py / call_consensus.py on the GPU box: the device's cell parser against Python's float() / int() bit for bit,
midas_sites_scan against the sequential model (tests/analyze_model.py) bit for bit at several group sizes, both commands
against the reference's own output (tests/golden/analyze_vectors.json), and the chain merge_midas.py snps -> snp_diversity.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

from midas_amd import abi
from midas_amd.analyze import synth
from tests import analyze_model as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    with abi.Context(0) as c:
        yield c


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _matrix(cells_by_row):
    return np.frombuffer(''.join('%d\t%s\n' % (r + 1, '\t'.join(row)) for r, row in enumerate(cells_by_row)).encode(), np.uint8)


# cells the device converts itself ...
FAST_FLOAT = ['0', '1', '0.5', '0.0123', '1e-05', '2.5e-05', '0.333', '0.667', '1.0', '0.0', '-0', '+0.25', '1E-3', '1e+2', '123456789.125',
              '9007199254740991', '0.9007199254740991', '1e22', '1e-22', '4.35', '0.1', '0.3', '8.5e-3', '0e999', '00.50', '7.0e-10',
              '9007199254740991e-22', '0.000000000000000000001', '5e-1']
# ... and cells it must pass to the host: long mantissas, big exponents, specials, separators, padding, odd shapes
SLOW_FLOAT = ['9007199254740993', '0.12345678901234567890', '1e23', '1e-23', '2.2250738585072014e-308', '1e400', '1e-400', 'nan', 'inf',
              '-inf', 'Infinity', '1_0.5', ' 0.5', '0.5 ', '.5', '5.', '1e0005', '4.9e-324', '17976931348623157e292', '0.1e-22', 'NaN']
FAST_INT = ['0', '1', '17', '+5', '-3', '007', '999999999999999999', '123456']
SLOW_INT = ['1_000', ' 12', '12 ', '9223372036854775807', '1234567890123456789', '-9223372036854775808']


def test_device_parser_is_float_and_int_bit_for_bit(ctx):
    rng = np.random.default_rng(11)
    S = 7
    fcells = FAST_FLOAT + SLOW_FLOAT + ['%.17g' % x for x in rng.random(40)] + ['%.3g' % x for x in rng.random(400)] + \
        ['%.6e' % x for x in rng.random(40) * 1e-5]
    icells = FAST_INT + SLOW_INT + [str(int(x)) for x in rng.integers(0, 100000, 400)]
    n = max(len(fcells), len(icells))
    n += (-n) % S
    fcells += ['0.25'] * (n - len(fcells))
    icells += ['3'] * (n - len(icells))
    order = rng.permutation(n)
    frows = [[fcells[k] for k in order[r * S:(r + 1) * S]] for r in range(n // S)]
    irows = [[icells[k] for k in order[r * S:(r + 1) * S]] for r in range(n // S)]
    N = n // S
    for group_rows, chunk in ((0, 0), (5, 256)):
        res = ctx.sites_scan(_matrix(frows), _matrix(irows), np.ones(N, np.uint8), np.arange(S), np.full(S, 10.0), 2, float('inf'), 0.5,
                             0.0, 0.0, group_rows=group_rows, chunk_bytes=chunk, dump=True)
        assert res['n_sites'] == N
        exp_f = np.array([[float(c) for c in row] for row in frows]).T
        exp_i = np.array([[int(c) for c in row] for row in irows], np.int64).T
        assert np.array_equal(_bits(res['freq']), _bits(exp_f))
        assert np.array_equal(res['depthv'], exp_i)
        assert res['side_freq'] == sum(not M.is_fast_float(c) for c in fcells)
        assert res['side_depth'] == sum(not M.is_fast_int(c) for c in icells)
        assert res['side_freq'] >= len(SLOW_FLOAT) and res['side_depth'] >= len(SLOW_INT)
    assert all(M.is_fast_float(c) for c in FAST_FLOAT) and not any(M.is_fast_float(c) for c in SLOW_FLOAT)
    assert all(M.is_fast_int(c) for c in FAST_INT) and not any(M.is_fast_int(c) for c in SLOW_INT)


@pytest.mark.parametrize("bad, where", [("0.5x", (1, 3, 2)), ("", (1, 3, 2)), ("1.0", (2, 3, 2)), ("abc", (2, 3, 2))])
def test_malformed_cells_and_short_rows_are_reported_with_their_place(ctx, bad, where):
    S, N = 4, 6
    frows = [['0.5'] * S for _ in range(N)]
    drows = [['5'] * S for _ in range(N)]
    (frows if where[0] == 1 else drows)[where[1]][where[2]] = bad
    args = (np.ones(N, np.uint8), np.arange(S), np.full(S, 10.0), 2, float('inf'), 0.5, 0.0, 0.0)
    with pytest.raises(abi.MidasSnpsError) as e:
        ctx.sites_scan(_matrix(frows), _matrix(drows), *args)
    assert e.value.bad == where
    # a column the sample filters dropped is never converted
    res = ctx.sites_scan(_matrix(frows), _matrix(drows), args[0], np.array([0, 1, 3]), np.full(3, 10.0), *args[3:])
    assert res['n_sites'] == N
    # a short row
    frows[where[1]][where[2]] = '0.5'
    drows[where[1]][where[2]] = '5'
    drows[4] = drows[4][:2]
    with pytest.raises(abi.MidasSnpsError) as e:
        ctx.sites_scan(_matrix(frows), _matrix(drows), *args)
    assert e.value.bad == (2, 4, -1)
    # ... beyond the row that fills --max_sites nothing is read
    res = ctx.sites_scan(_matrix(frows), _matrix(drows), *args, max_sites=2)
    assert res['n_kept'] == 2


def test_a_column_selected_twice_is_refused_even_where_there_is_no_row(ctx):
    none, cols = np.zeros(0, np.uint8), np.array([0, 0])
    calls = [lambda: ctx.sites_scan(none, none, none, cols, np.full(2, 10.0), 2, float('inf'), 0.5, 0.0, 0.0),
             lambda: ctx.sites_id_markers(none, none, none, none, cols, 0.1, 3, 1),
             lambda: ctx.sites_track_markers(none, none, none, cols, 0.1, 3),
             lambda: ctx.sites_consensus_pairs(none, none, none, cols, np.full(2, 10.0), 2, float('inf'), 0.5, 0.0, 0.0)]
    for call in calls:
        with pytest.raises(abi.MidasSnpsError) as e:
            call()
        assert e.value.status == abi.ERR_INVALID_ARG and 'selected twice' in str(e.value) and e.value.bad is None


def _species(tmp_path_factory, n_sites, n_samples, seed, n_genes):
    d = str(tmp_path_factory.mktemp("sp") / "species_1")
    synth.write_species_dir(d, n_sites, n_samples, seed=seed, n_genes=n_genes, block=7000)
    return abi.SitesTables(d)


MODES = [
    dict(flags=abi.SITES_SUMS),
    dict(flags=abi.SITES_SUMS | abi.SITES_PER_GENE),
    dict(flags=abi.SITES_SUMS | abi.SITES_POOLED, site_prev=0.3),
    dict(flags=abi.SITES_SUMS | abi.SITES_POOLED | abi.SITES_PER_GENE | abi.SITES_WEIGHT, site_maf=0.01),
    dict(flags=abi.SITES_SUMS | abi.SITES_ROUND, allele_support=0.7, site_ratio=2.0),
    dict(flags=abi.SITES_SUMS | abi.SITES_POOLED | abi.SITES_PER_GENE | abi.SITES_ROUND, max_sites=3000),
    dict(flags=abi.SITES_SEQ, site_prev=0.5, site_depth=3),
    dict(flags=abi.SITES_SEQ | abi.SITES_MASK_ONLY, max_sites=777),
]


def _same(a, b, what):
    for k in ('n_kept', 'side_freq', 'side_depth', 'no_gene'):
        assert a[k] == b[k], (what, k, a[k], b[k])
    for k in ('snps', 'sites', 'depth', 'seq', 'keep', 'depthv'):
        if k in b:
            assert np.array_equal(a[k], b[k]), (what, k)
    for k in ('pi', 'pooled', 'freq'):
        if k in b:
            assert np.array_equal(_bits(a[k]), _bits(b[k])), (what, k)


@pytest.mark.parametrize("n_samples", [13, 150])
def test_scan_matches_the_sequential_model_at_every_group_size(ctx, tmp_path_factory, n_samples):
    n_sites = 12000 if n_samples == 13 else 2500
    t = _species(tmp_path_factory, n_sites, n_samples, seed=n_samples, n_genes=37)
    rng = np.random.default_rng(5)
    mask = (rng.random(n_sites) < 0.9).astype(np.uint8)
    cols = np.array([c for c in range(n_samples) if c % 5 != 3])
    mean = t.mean_coverage[cols]
    minor, _ = t.first_bytes('minor_allele')
    major, _ = t.first_bytes('major_allele')
    for mode in MODES:
        kw = dict(site_depth=2, site_ratio=float('inf'), allele_support=0.5, site_prev=0.0, site_maf=0.0, snp_maf=0.01, max_sites=-1,
                  site_gene=t.gene, n_genes=t.n_genes, minor=minor, major=major)
        kw.update(mode)
        exp = M.sites_scan(t.freq_text, t.depth_text, mask, cols, mean, dump=True, **kw)
        groups = []
        for group_rows, chunk in ((0, 0), (1000, 0), (777, 100000)):
            got = ctx.sites_scan(t.freq_text, t.depth_text, mask, cols, mean, group_rows=group_rows, chunk_bytes=chunk, dump=True, **kw)
            if kw['max_sites'] >= 0:      # (the device reads whole groups, the model stops where the loop stops: no dumps)
                skip = ('freq', 'depthv', 'keep', 'pooled', 'side_freq', 'side_depth')
                got = dict({k: v for k, v in got.items() if k not in skip}, side_freq=0, side_depth=0)
                _same(got, dict({k: v for k, v in exp.items() if k not in skip}, side_freq=0, side_depth=0), (mode, group_rows))
            else:
                _same(got, exp, (mode, group_rows))
                assert got['side_freq'] == 0 and got['side_depth'] == 0      # '{:.3g}' cells all fit the device's converter
            groups.append(got['groups'])
        assert kw['max_sites'] >= 0 or (groups[0] == 1 and groups[1] > 1 and groups[2] >= groups[1]), groups


# ---- the commands ----------------------------------------------------------------------------------------------------------------
from midas_amd import synth as reads_synth                                            # noqa: E402
from midas_amd.analyze import sites as host_sites                                     # noqa: E402
from tests import test_analyze_host as H                                              # noqa: E402

VEC = M.load_vectors()


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("analyze_gpu"))
    for name, sp in VEC['species'].items():
        H._write_species('%s/%s' % (tmp, name), sp)
    for name, text in VEC['site_lists'].items():
        with open('%s/%s.list' % (tmp, name), 'w') as f:
            f.write(text)
    return tmp


class _Shared:
    """The module's context, handed to run_pipeline: its close() leaves the context to the fixture."""

    def __init__(self, ctx):
        self._ctx = ctx

    def sites_scan(self, *a, **kw):
        return self._ctx.sites_scan(*a, **kw)

    def close(self):
        pass


@pytest.mark.parametrize("k", range(len(VEC['diversity'])))
def test_snp_diversity_on_the_device_writes_the_references_bytes(ctx, tree, tmp_path, k):
    H.check_diversity_case(tree, VEC['diversity'][k], str(tmp_path / 'pi.txt'), make_context=lambda: _Shared(ctx))


@pytest.mark.parametrize("k", range(len(VEC['consensus'])))
def test_call_consensus_on_the_device_writes_the_references_bytes(ctx, tree, tmp_path, k):
    H.check_consensus_case(tree, VEC['consensus'][k], str(tmp_path / 'seqs.fa'), make_context=lambda: _Shared(ctx))


def _script(name, *argv):
    return subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', name)] + list(argv), capture_output=True, text=True, cwd=ROOT)


def test_the_scripts_themselves_against_the_golden(tree, tmp_path):
    """The real command lines, each in its own process (no seeded case: a child cannot share the parent's random stream)."""
    for script, cases in (('snp_diversity.py', [c for c in VEC['diversity'] if c['seed'] is None][:4]), ('call_consensus.py', VEC['consensus'][:2])):
        for case in cases:
            out = str(tmp_path / 'out.txt')
            r = _script(script, *H._argv(tree, case, out), '--group_rows', '17')
            assert r.returncode == 0, r.stderr + r.stdout
            per_gene = 'per-gene' in case['options']
            assert H._rows(open(out).read(), per_gene) == H._rows(case['out'], per_gene)
            assert "Script: %s" % script in r.stdout


def test_merge_midas_snps_then_snp_diversity(ctx, tmp_path):
    """The chain: this project's own merge writes the tables, every cell of which the device converts itself (zero cells for
    the host: '{:.3g}' always fits), and the command's output is the sequential model's on the same directory."""
    data = reads_synth.make_merge_dataset(str(tmp_path / "samples"), n_samples=5, n_sites=6000, seed=11)
    merged = str(tmp_path / "merged")
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'merge_midas.py'), 'snps', merged, '-i', os.path.dirname(data['samples'][0]),
                        '-t', 'dir', '-d', data['db'], '--all_sites'], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr + r.stdout
    d = os.path.join(merged, 'sp1')
    t = abi.SitesTables(d)
    assert t.n_sites > 1000 and t.n_samples == 5
    res = ctx.sites_scan(t.freq_text, t.depth_text, host_sites.info_mask(t), np.arange(5), t.mean_coverage, 2, float('inf'), 0.5, 0.0, 0.0,
                         flags=abi.SITES_SUMS)
    assert res['n_sites'] == t.n_sites and res['side_freq'] == 0 and res['side_depth'] == 0
    for opts in ([], ['--sample_type', 'pooled-samples', '--site_prev', '0.5', '--weight_by_depth']):
        out, exp = str(tmp_path / 'pi.txt'), str(tmp_path / 'pi_model.txt')
        r = _script('snp_diversity.py', d, '--out', out, *opts)
        assert r.returncode == 0, r.stderr + r.stdout
        H._run('snp_diversity.py', merged, dict(species='sp1', options=opts), exp)
        assert open(out).read() == open(exp).read() and len(open(out).read().splitlines()) >= 2
    out, exp = str(tmp_path / 'seq.fa'), str(tmp_path / 'seq_model.fa')
    r = _script('call_consensus.py', d, '--out', out, '--site_prev', '0.5')
    assert r.returncode == 0, r.stderr + r.stdout
    H._run('call_consensus.py', merged, dict(species='sp1', options=['--site_prev', '0.5']), exp)
    assert open(out).read() == open(exp).read()
