"""The per-site kernels (sites_rows.h, sites_call.h, sites_scan.hip, sites_strains.hip) on the GPU box, on the chosen tables of tests/site_cases.py: every decision of the site
loop on its border and to either side of it, the pooled frequency at every change of the pairwise reduce's shape, the sums at
every place a gene can change, the marker calls at their rounding cases and the device's own converters at the ends of their
fast paths -- device against the sequential models, bit for bit, with one row group and with several.  Where the model raises
(the reference would), the device call must refuse, with the model's reason, row and sample.
tests/test_site_cases_host.py shows, without a GPU, that every case sits where its name says."""
import numpy as np
import pytest

from midas_amd import abi
from tests import analyze_model as M
from tests import site_cases as C
from tests import snp_trees_model as TM
from tests import strains_model as T
from tests import test_analyze_host as H

pytestmark = pytest.mark.gpu
CASES = C.site_cases(M.pairwise_sum)
BY_NAME = {c.name: c for c in CASES}
MARKERS = C.marker_cases()
GROUPS = ((0, 0), (3, 0), (1, 256))          # one group; a few rows a group; a group a row, chunks that have to grow


@pytest.fixture(scope="module")
def ctx():
    with abi.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def expected():
    """The model's answer to every case, formed once: a result, or the BadCell it raises."""
    out = {}
    for c in CASES:
        try:
            out[c.name] = C.run(M.sites_scan, c)
        except M.BadCell as e:
            out[c.name] = e
    return out


def _bits(a):
    """The bit patterns; every NaN as one pattern (which NaN an operation returns is not the arithmetic's to say: the sign and
    the payload of a NaN that inf - inf or nan + x produces differ between processors)."""
    a = np.ascontiguousarray(a, np.float64)
    return np.where(np.isnan(a), np.uint64(0x7FF8000000000000), a.view(np.uint64))


def _same(got, exp, what, whole):
    """whole: no --max_sites, so the device reads the rows the model reads and the dumps and side counts compare too."""
    assert got['n_kept'] == exp['n_kept'] and got['no_gene'] == exp['no_gene'], what
    for k in ('snps', 'sites', 'depth', 'seq'):
        if k in exp:
            assert np.array_equal(got[k], exp[k]), (what, k)
    if 'pi' in exp:
        assert np.array_equal(_bits(got['pi']), _bits(exp['pi'])), (what, 'pi')
    n = len(got['keep'])
    assert np.array_equal(got['keep'], exp['keep'][:n]) and not exp['keep'][n:].any(), (what, 'keep')
    if whole:
        assert got['n_sites'] == exp['n_sites'] and got['side_freq'] == exp['side_freq'] and got['side_depth'] == exp['side_depth'], what
        assert np.array_equal(got['depthv'], exp['depthv']), (what, 'depthv')
        for k in ('pooled', 'freq'):
            assert np.array_equal(_bits(got[k]), _bits(exp[k])), (what, k)


@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_site_case_equals_the_model_at_every_group_setting(ctx, expected, name):
    c, exp = BY_NAME[name], expected[name]
    for group_rows, chunk in GROUPS + c.note['groups']:
        what = (name, group_rows, chunk)
        if isinstance(exp, M.BadCell):
            with pytest.raises(abi.MidasSnpsError) as e:
                C.run(ctx.sites_scan, c, group_rows=group_rows, chunk_bytes=chunk)
            assert e.value.status == abi.ERR_BAD_LAYOUT and e.value.bad == exp.bad, what
            continue
        got = C.run(ctx.sites_scan, c, group_rows=group_rows, chunk_bytes=chunk)
        _same(got, exp, what, c.opts['max_sites'] < 0)
        if c.opts['max_sites'] < 0:
            assert got['groups'] == (1 if group_rows == 0 else -(-len(c.frows) // group_rows)), what


SMALL = [c.name for c in CASES if len(c.cols) <= 40]


@pytest.mark.parametrize("name", SMALL)
def test_consensus_planes_of_the_site_case_equal_the_model(ctx, name):
    """midas_sites_consensus_pairs makes the same site decisions (unweighted, unrounded) and turns ss_seq_kernel's letters into
    the `called` and `minor` planes: its pair counts against the model's, which counts the letters of the model's sequences."""
    c = BY_NAME[name]
    o = c.opts
    args = (C.matrix(c.frows), C.matrix(c.drows), c.mask, c.cols, c.mean, o['site_depth'], o['site_ratio'], o['allele_support'], o['site_prev'],
            o['site_maf'])
    kw = dict(max_sites=o['max_sites'], flags=o['flags'])
    try:
        exp = TM.sites_consensus_pairs(*args, **kw)
    except M.BadCell as e:
        exp = e
    for group_rows, chunk in GROUPS + c.note['groups']:
        if isinstance(exp, M.BadCell):
            with pytest.raises(abi.MidasSnpsError) as e:
                ctx.sites_consensus_pairs(*args, group_rows=group_rows, chunk_bytes=chunk, **kw)
            assert e.value.bad == exp.bad, (name, group_rows)
            continue
        got = ctx.sites_consensus_pairs(*args, group_rows=group_rows, chunk_bytes=chunk, **kw)
        assert got['n_kept'] == exp['n_kept'], (name, group_rows)
        assert np.array_equal(np.triu(got['both']), exp['both']) and np.array_equal(np.triu(got['diff']), exp['diff']), (name, group_rows)


@pytest.mark.parametrize("name", [m.name for m in MARKERS])
def test_marker_case_equals_the_model_at_every_group_setting(ctx, name):
    m = [x for x in MARKERS if x.name == name][0]
    f, d, cols = C.matrix(m.frows), C.matrix(m.drows), np.arange(len(m.frows[0]))
    n = len(m.frows)
    exp = T.sites_id_markers(f, d, m.minor, m.major, cols, m.min_freq, m.min_reads, m.allele_prev)
    whiches = [np.full(n, 2, np.uint8), np.full(n, 1, np.uint8), (np.arange(n) % 3).astype(np.uint8)]
    exp_t = [T.sites_track_markers(f, d, w, cols, m.min_freq, m.min_reads) for w in whiches]
    for group_rows, chunk in GROUPS:
        got = ctx.sites_id_markers(f, d, m.minor, m.major, cols, m.min_freq, m.min_reads, m.allele_prev, group_rows=group_rows, chunk_bytes=chunk)
        assert np.array_equal(got['rows'], exp['rows']), (name, group_rows)
        assert got['n_sites'] == n and got['side_freq'] == exp['side_freq'] and got['side_depth'] == exp['side_depth']
        for w, e in zip(whiches, exp_t):
            got_t = ctx.sites_track_markers(f, d, w, cols, m.min_freq, m.min_reads, group_rows=group_rows, chunk_bytes=chunk)
            assert np.array_equal(np.triu(got_t['both']), e['both']) and got_t['n_matched'] == e['n_matched'], (name, group_rows)


# ---- the device's own converters ----------------------------------------------------------------------------------------------------
def _table(cells, S, pad):
    cells = list(cells) + [pad] * ((-len(cells)) % S)
    return [cells[r * S:(r + 1) * S] for r in range(len(cells) // S)]


def test_converters_at_the_borders_of_their_fast_paths(ctx):
    S = 7
    fcells, icells = [c for c, _ in C.float_cells()], [c for c, _ in C.int_cells()]
    frows = _table(fcells, S, '0.25')
    irows = _table(icells + ['3'] * (len(frows) * S - len(icells)), S, '3')
    N = len(frows)
    assert len(irows) == N
    args = (np.ones(N, np.uint8), np.arange(S), np.full(S, 10.0), 2, float('inf'), 0.5, 0.0, 0.0)
    for group_rows, chunk in GROUPS + ((5, 256),):
        res = ctx.sites_scan(C.matrix(frows), C.matrix(irows), *args, group_rows=group_rows, chunk_bytes=chunk, dump=True)
        assert res['n_sites'] == N
        exp_f = np.array([[float(c) for c in row] for row in frows]).T
        exp_i = np.array([[int(c) for c in row] for row in irows], np.int64).T
        wrong = np.argwhere(res['freq'].view(np.uint64) != exp_f.view(np.uint64))
        assert wrong.shape[0] == 0, [frows[r][s] for s, r in wrong.tolist()]
        assert np.array_equal(res['depthv'], exp_i)
        assert res['side_freq'] == sum(not M.is_fast_float(c) for row in frows for c in row) == sum(not fast for _, fast in C.float_cells())
        assert res['side_depth'] == sum(not M.is_fast_int(c) for row in irows for c in row) == sum(not fast for _, fast in C.int_cells())
    # spellings that float() / int() refuse: the device hands them to the host, which refuses them with their place
    for which, refused in ((1, C.REFUSED_FLOATS), (2, C.REFUSED_INTS)):
        for k, cell in enumerate(refused):
            fr, ir = [['0.5'] * S for _ in range(6)], [['5'] * S for _ in range(6)]
            r, s = k % 6, (3 * k) % S
            (fr if which == 1 else ir)[r][s] = cell
            with pytest.raises(abi.MidasSnpsError) as e:
                ctx.sites_scan(C.matrix(fr), C.matrix(ir), np.ones(6, np.uint8), *args[1:], group_rows=(0, 2)[k % 2])
            assert e.value.bad == (which, r, s), cell


# ---- the commands: a site the reference raises on ends them with the file, the line and the sample ------------------------------------
class _Shared:
    def __init__(self, ctx):
        self._ctx = ctx

    def sites_scan(self, *a, **kw):
        return self._ctx.sites_scan(*a, **kw)

    def close(self):
        pass


def test_snp_diversity_consensus_exits_on_a_frequency_it_cannot_round(ctx, tmp_path):
    d = str(tmp_path / 'ragged')
    H._write_species(d, C.with_cell(H.VEC['species']['ragged'], 'freq', 7, 3, 'nan'))
    for extra in ([], ['--group_rows', '3']):
        with pytest.raises(SystemExit) as e:
            H._run('snp_diversity.py', str(tmp_path), dict(species='ragged', options=['--consensus'] + extra), str(tmp_path / 'o'),
                   make_context=lambda: _Shared(ctx))
        assert e.value.code == C.ROUND_EXIT % (d, 8, 's002')
    # without --consensus nothing is rounded: the reference goes on, and so do the device and the model, to the same bytes
    out, exp = str(tmp_path / 'pi.txt'), str(tmp_path / 'pi_model.txt')
    H._run('snp_diversity.py', str(tmp_path), dict(species='ragged', options=[]), out, make_context=lambda: _Shared(ctx))
    H._run('snp_diversity.py', str(tmp_path), dict(species='ragged', options=[]), exp)
    assert open(out).read() == open(exp).read()
