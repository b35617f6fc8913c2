"""snp_diversity.py --rand_reads on the GPU box: the device's MT19937 generator against numpy's from the same state, word for word
and state for state; midas_sites_scan_resampled against the sequential model (tests/resample_model.py) bit for bit at every
group size, launch size and start position; and the command against the reference's own output and final generator state
(tests/golden/resample_vectors.json)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from midas_amd import abi
from tests import resample_model as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VEC = M.load_vectors()
CASES = VEC['cases']


@pytest.fixture(scope="module")
def ctx():
    with abi.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return M.write_tree(str(tmp_path_factory.mktemp("resample_gpu")), VEC)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _state_at(seed, pos):
    """numpy's legacy state after np.random.seed(seed), moved to position pos of a block (624: as seeded; 0: set by hand)."""
    np.random.seed(seed)
    if pos == 0:
        st = np.random.get_state()
        return ('MT19937', st[1], 0, 0, 0.0)
    if pos != 624:
        np.random.randint(0, 2 ** 32, pos, dtype=np.uint32)          # a refill, then pos words
    st = np.random.get_state()
    assert int(st[2]) == pos
    return st


def _numpy_words(state, n):
    bg = np.random.MT19937()
    bg.state = dict(bit_generator='MT19937', state=dict(key=np.array(state[1], np.uint32), pos=int(state[2])))
    raw = bg.random_raw(n).astype(np.uint32)
    return raw, bg.state['state']


# ---- the generator alone ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pos", [624, 623, 0, 311])
def test_the_generator_continues_numpys_stream(ctx, pos):
    n = 3 * 624 + 5
    state = _state_at(40 + pos, pos)
    exp, end = _numpy_words(state, n)
    for per_launch, bound in ((0, 8), (700, 32), (1, 0)):
        m = n if per_launch != 1 else 7
        raw, flag, masked, key, at = ctx.mt19937_stream(state[1], pos, m, per_launch=per_launch, bound=bound)
        assert np.array_equal(raw, exp[:m]), (pos, per_launch)
        mask = M.draw_mask(bound + 1)
        assert np.array_equal(masked, exp[:m] & np.uint32(mask)) and np.array_equal(flag, (exp[:m] & np.uint32(mask)) <= bound)
        want = end if m == n else _numpy_words(state, m)[1]
        assert at == int(want['pos']) and np.array_equal(key, want['key']), (pos, per_launch)
    # no word: the state as given
    raw, _, _, key, at = ctx.mt19937_stream(state[1], pos, 0)
    assert raw.size == 0 and at == pos and np.array_equal(key, np.asarray(state[1], np.uint32))


# ---- the resampled scan against the model ---------------------------------------------------------------------------------------------
SPECIES = {'a13': 60, 'b150': 40}           # sites in use


def _same(got, exp, what):
    for k in ('n_kept', 'n_resampled', 'n_drew', 'raw_consumed'):
        assert got[k] == exp[k], (what, k, got[k], exp[k])
    for k in ('snps', 'sites', 'depth', 'keep', 'depthv'):
        assert np.array_equal(got[k], exp[k]), (what, k)
    for k in ('pi', 'pooled', 'freq'):
        assert np.array_equal(_bits(got[k]), _bits(exp[k])), (what, k)
    assert int(got['np_state'][2]) == int(exp['np_state'][2]) and np.array_equal(got['np_state'][1], exp['np_state'][1]), what


@pytest.mark.parametrize("n_reads", [1, 2, 3, 8, 9, 33])
@pytest.mark.parametrize("species", sorted(SPECIES))
def test_resampled_scan_matches_the_model_whatever_the_groups_and_launches(ctx, tree, species, n_reads):
    t = abi.SitesTables('%s/%s' % (tree, species))
    n_sites = SPECIES[species]
    cols = np.arange(t.n_columns)
    mean = t.mean_coverage[cols]
    flags = abi.SITES_SUMS | (0 if n_reads % 2 else abi.SITES_POOLED | abi.SITES_WEIGHT)
    kw = dict(site_depth=max(2, n_reads), site_ratio=float('inf'), allele_support=0.5, site_prev=0.0, site_maf=0.0, flags=flags,
              rand_reads=n_reads, replace_reads=True, dump=True)
    mask = np.ones(n_sites, np.uint8)
    for pos, shapes in ((624, [(g, c) for g in (1, 7, 64, 0) for c in (624, 1000, 0)]), (311, [(7, 624), (0, 0)])):
        state = _state_at(7 * n_reads + len(species), pos)
        exp = M.sites_scan(t.freq_text, t.depth_text, mask, cols, mean, np_state=state, **kw)
        assert exp['n_resampled'] > 10 and exp['n_drew'] > 50 and (exp['raw_consumed'] > 0) == (n_reads > 1)
        assert (exp['depthv'][:, exp['keep'] == 1] == n_reads).any() and (exp['depthv'] != n_reads).any()
        for group_rows, chunk in shapes:
            got = ctx.sites_scan(t.freq_text, t.depth_text, mask, cols, mean, np_state=state, group_rows=group_rows, draw_chunk=chunk, **kw)
            _same(got, exp, (species, n_reads, pos, group_rows, chunk))
            assert got['accepted_used'] == (exp['n_drew'] * n_reads if n_reads > 1 else 0)
            assert got['raw_made'] >= got['raw_consumed']
            assert got['groups'] == (n_sites if group_rows == 1 else -(-n_sites // group_rows) if group_rows else 1)


@pytest.mark.parametrize("species", sorted(SPECIES))
def test_without_replacement_is_the_closed_form_and_takes_no_word(ctx, tree, species):
    t = abi.SitesTables('%s/%s' % (tree, species))
    n_sites, n_reads = SPECIES[species], 5
    cols = np.arange(t.n_columns)
    mean = t.mean_coverage[cols]
    mask = np.ones(n_sites, np.uint8)
    state = _state_at(9, 311)
    args = (t.freq_text, t.depth_text, mask, cols, mean, n_reads, float('inf'), 0.5, 0.0, 0.0)
    plain = ctx.sites_scan(*args, flags=abi.SITES_SUMS, dump=True)
    got = ctx.sites_scan(*args, flags=abi.SITES_SUMS, dump=True, rand_reads=n_reads, replace_reads=False, np_state=state, group_rows=7)
    exp = M.sites_scan(*args, flags=abi.SITES_SUMS, dump=True, rand_reads=n_reads, replace_reads=False, np_state=state)
    _same(got, exp, species)
    assert got['raw_made'] == 0 and got['raw_consumed'] == 0 and int(got['np_state'][2]) == 311 and np.array_equal(got['np_state'][1], state[1])
    redo = (plain['keep'] == 1) & (plain['pooled'] > 0)
    assert redo.any() and not redo.all() and got['n_resampled'] == int(redo.sum())
    f = plain['freq'][:, redo]
    closed = np.where((f > 0) & (f < 1), np.rint(f * n_reads) / n_reads, f)
    assert np.array_equal(_bits(got['freq'][:, redo]), _bits(closed)) and (got['depthv'][:, redo] == n_reads).all()
    assert np.array_equal(_bits(got['freq'][:, ~redo]), _bits(plain['freq'][:, ~redo])) and np.array_equal(got['depthv'][:, ~redo], plain['depthv'][:, ~redo])
    assert (np.rint(0.5 * n_reads) == 2) and (closed == 0.4).any()           # 0.5 x 5 = 2.5 goes to 2


def test_the_option_has_no_place_in_call_consensus(ctx, tree):
    t = abi.SitesTables('%s/a13' % tree)
    minor, _ = t.first_bytes('minor_allele')
    major, _ = t.first_bytes('major_allele')
    with pytest.raises(abi.MidasSnpsError) as e:
        ctx.sites_scan(t.freq_text, t.depth_text, np.ones(t.n_sites, np.uint8), np.arange(13), t.mean_coverage, 5, float('inf'), 0.5, 0.0, 0.0,
                       flags=abi.SITES_SEQ, minor=minor, major=major, rand_reads=5, replace_reads=True, np_state=_state_at(1, 624))
    assert e.value.status == abi.ERR_INVALID_ARG


# ---- the command ------------------------------------------------------------------------------------------------------------------
class _Shared:
    """The module's context, handed to run_pipeline: its close() leaves the context to the fixture."""

    def __init__(self, ctx):
        self._ctx = ctx

    def sites_scan(self, *a, **kw):
        return self._ctx.sites_scan(*a, **kw)

    def close(self):
        pass


@pytest.mark.parametrize("k", range(len(CASES)))
def test_snp_diversity_on_the_device_writes_the_references_bytes_and_leaves_its_state(ctx, tree, tmp_path, k):
    M.check_case(tree, CASES[k], str(tmp_path / 'pi.txt'), make_context=lambda: _Shared(ctx), extra=['--group_rows', '17'] if k % 2 else [])


def test_the_script_itself_with_seed_against_the_golden(tree, tmp_path):
    case = [c for c in CASES if c['seed'] == 3][0]
    assert case['options'] == ['--rand_reads', '9', '--replace_reads']
    out = str(tmp_path / 'out.txt')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'snp_diversity.py'), '%s/%s' % (tree, case['species'])] + case['options'] +
                       ['--seed', '3', '--out', out], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    assert open(out).read() == case['out']
    assert '  rand_reads: 9\n  replace_reads: True\n' in r.stdout and '  site_depth: 9\n' in r.stdout
