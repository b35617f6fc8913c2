"""The chosen tables of tests/site_cases.py, checked with the sequential models alone (no GPU): every case sits where its name
says -- on its border, or on the named side of it -- so that none can quietly stop testing anything."""
import numpy as np
import pytest

from midas_amd import abi
from tests import analyze_model as M
from tests import site_cases as C
from tests import strains_model as T

CASES = C.site_cases(M.pairwise_sum)
BY_NAME = {c.name: c for c in CASES}
MARKERS = C.marker_cases()


def run_model(c, rows=None, **over):
    return C.run(M.sites_scan, c, rows, **over)


def sample_keep(c, r):
    """Which samples the model keeps at row r: the per-sample site counts of that row alone, no site filter."""
    res = run_model(c, [r], flags=C.SUMS, site_prev=0.0, site_maf=0.0, max_sites=-1)
    return [bool(x) for x in res['sites'][:, 0]]


def test_the_flags_are_the_librarys():
    assert (C.WEIGHT, C.ROUND, C.POOLED, C.PER_GENE, C.MASK_ONLY, C.SEQ, C.SUMS) == \
        (abi.SITES_WEIGHT, abi.SITES_ROUND, abi.SITES_POOLED, abi.SITES_PER_GENE, abi.SITES_MASK_ONLY, abi.SITES_SEQ, abi.SITES_SUMS)
    assert len(BY_NAME) == len(CASES)
    assert sorted(c.note['pairwise'] for c in CASES if 'pairwise' in c.note and not c.name.endswith('_round')) == sorted(C.PAIRWISE_COUNTS)


@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_the_case_sits_where_its_name_says(name):
    c = BY_NAME[name]
    note = c.note
    if note.get('raises'):
        with pytest.raises(M.BadCell) as e:
            run_model(c)
        assert e.value.bad == note['raises'] and e.value.status == abi.ERR_BAD_LAYOUT
        return
    res = run_model(c)
    S = len(c.cols)
    if 'kept' in note:
        assert sample_keep(c, 0) == note['kept']
    for cell in note.get('f_on', ()):                 # the frequency, or one minus it, is the support itself
        assert float(cell) == c.opts['allele_support'] and sample_keep(c, 0)[c.frows[0].index(cell)]
    for cell in note.get('q_on', ()):
        assert 1 - float(cell) == c.opts['allele_support'] and sample_keep(c, 0)[c.frows[0].index(cell)]
    for d, mean, want in note.get('ratio', ()):
        q, ratio = d / mean, c.opts['site_ratio']
        assert q == dict(on=ratio, over=C.up(ratio), under=C.down(ratio))[want] and (q > ratio) == (want == 'over')
    if 'site_keep' in note:
        assert res['keep'].tolist() == [int(k) for k in note['site_keep']]
    if 'counts' in note:
        assert [sum(sample_keep(c, r)) for r in range(len(c.frows))] == note['counts']
    if 'on' in note:
        k, n, prev = note['on']
        assert n == S and k / n == prev == c.opts['site_prev']
    if 'pool' in note:
        maf, wants = note['pool']
        for r, want in enumerate(wants):
            assert res['pooled'][r] == dict(on=maf, over=C.up(maf), under=C.down(maf))[want]
    for r in note.get('pooled0', ()):
        assert C.bits(res['pooled'][r]) == C.bits(0.0) and sum(sample_keep(c, r)) == 0
    if 'pairwise' in note:
        K = note['pairwise']
        for r in range(len(c.frows)):
            keep = sample_keep(c, r)
            kept = [float(c.frows[r][s]) for s in range(S) if keep[s]]
            assert len(kept) == K
            on = [s for s in range(S) if keep[s]]
            if r == 0:              # the dropped samples in front of, behind and between the kept ones
                assert on[0] >= 3 and on[-1] - on[0] == K - 1
            elif r == 1:
                assert on[0] == 0 and on[-1] == K - 1 < S - 3
            else:
                assert on[-1] - on[0] > K - 1 or K == 1
            if K >= 8:
                assert C.bits(M.pairwise_sum(kept)) != C.bits(C.sequential_sum(kept))
            if not c.opts['flags'] & C.ROUND:
                assert C.bits(res['pooled'][r]) == C.bits(M.pairwise_sum(kept) / K)
    for r in note.get('weighted_order', ()):
        terms = [int(d) * float(f) for f, d in zip(c.frows[r], c.drows[r])]
        assert C.sequential_sum(terms) != C.sequential_sum(terms[::-1])
    if note.get('rounds'):
        assert [float(round(float(x))) for x in C.ROUND_CELLS] == C.ROUND_TO
        if c.opts['flags'] & C.SEQ:
            assert bytes(res['seq'][:, 0]) == b'aabaab--b'
    for r, value in note.get('pooled_bits', ()):
        assert C.bits(res['pooled'][r]) == C.bits(value)
    if 'fill' in note:
        assert res['n_kept'] == min(note['fill'], int(c.mask.sum()))
    if note.get('genes') and c.opts['flags'] & C.PER_GENE:
        gene, keep = c.opts['site_gene'], res['keep'].astype(bool)
        assert res['no_gene'] == int((keep & (gene < 0)).sum()) > 0
        assert all(keep[r] for r in (63, 64, 100))                       # the rows where the gene changes at lane 63 and at lane 0
        assert res['sites'][0].tolist()[4] == 0 and res['sites'].shape == (1 if c.opts['flags'] & C.POOLED else S, 5)
        assert (np.diff(np.flatnonzero(gene == 0)) > 1).any() and int((gene == 2).sum()) == 1        # a gene that comes back; one of one site
    if 'snp' in note:
        assert [int(run_model(c, [r])['snps'][0, 0]) for r in range(len(c.frows))] == [int(x) for x in note['snp']]
    if note.get('fma') == 'pi':
        fs = [float(row[0]) for row in c.frows]
        assert C.bits(C.pi_chain(fs, False)) == C.bits(res['pi'][0, 0]) != C.bits(C.pi_chain(fs, True))
    if note.get('fma') == 'pooled':
        fs = res['pooled'].tolist()
        assert C.bits(C.pi_chain(fs, False)) == C.bits(res['pi'][0, 0]) != C.bits(C.pi_chain(fs, True))
    if note.get('fma') == 'msum':
        plain = contracted = 0.0
        dsum = 0
        for f, d in zip(c.frows[0], c.drows[0]):
            plain += int(d) * float(f)
            contracted = C.fused(float(int(d)), float(f), contracted)
            dsum += int(d)
        assert C.bits(plain / dsum) == C.bits(res['pooled'][0]) != C.bits(contracted / dsum)
    if 'depth_sum' in note:
        assert (res['depth'][:, 0] > note['depth_sum']).all()


def _marker_model(m, **over):
    kw = dict(min_freq=m.min_freq, min_reads=m.min_reads, allele_prev=m.allele_prev)
    kw.update(over)
    return T.sites_id_markers(C.matrix(m.frows), C.matrix(m.drows), m.minor, m.major, np.arange(len(m.frows[0])), **kw)


@pytest.mark.parametrize("name", [m.name for m in MARKERS])
def test_the_marker_case_sits_where_its_name_says(name):
    m = [x for x in MARKERS if x.name == name][0]
    rows = _marker_model(m)['rows']
    note = m.note
    if 'product' in note:
        f, d, prod, r = note['product']
        assert float(f) * d == prod and round(float(f) * d) == r
    if 'has_minor' in note or 'has_major' in note:
        assert rows[:, 0].tolist() == list(range(len(m.frows)))          # every site is reported: the counts show sample 0's calls
        mi, ma = int(m.minor[0]), int(m.major[0])
        if 'has_minor' in note:
            assert (rows[:, 3 + mi] - 1).tolist() == [int(x) for x in note['has_minor']]
        if 'has_major' in note:
            assert (rows[:, 3 + ma] - 1).tolist() == [int(x) for x in note['has_major']]
    if 'total' in note:
        assert rows[:, 2].tolist() == note['total']
    if 'markers' in note:
        assert rows[:, 0].tolist() == [r for r, on in enumerate(note['markers']) if on]


def test_the_converter_cells_are_classified_as_their_lists_say():
    for cell, fast in C.float_cells():
        assert M.is_fast_float(cell) == fast, cell
        assert abi.parse_cell(cell.encode(), 'freq') == float(cell), cell
    for cell, fast in C.int_cells():
        assert M.is_fast_int(cell) == fast, cell
        assert abi.parse_cell(cell.encode(), 'depth') == int(cell), cell
    for cell in C.REFUSED_FLOATS:
        with pytest.raises(ValueError):
            float(cell)
        assert not M.is_fast_float(cell) and abi.parse_cell(cell.encode(), 'freq') is None, cell
    for cell in C.REFUSED_INTS:
        with pytest.raises(ValueError):
            int(cell)
        assert not M.is_fast_int(cell) and abi.parse_cell(cell.encode(), 'depth') is None, cell
    lim = 1 << 53
    cells = dict(C.float_cells())
    assert cells[str(lim - 1)] and not cells[str(lim)] and cells['1.5e23'] and not cells['1e23'] and not cells['0.50000000000000000000']
    assert sum(fast for _, fast in C.float_cells()) > 100 and sum(not fast for _, fast in C.float_cells()) > 40


# ---- the commands: a site the reference raises on ends them with the file, the line and the sample ------------------------------------
from tests import snp_trees_model as TM                                               # noqa: E402
from tests import test_analyze_host as H                                              # noqa: E402
from tests import test_snp_trees_host as HT                                           # noqa: E402


class _Refusing:
    """A context whose calls refuse as the device does for a site it cannot pool."""

    def __init__(self, bad):
        self.bad = bad

    def _refuse(self, *a, **kw):
        raise M.BadCell(self.bad, "refused")

    sites_scan = sites_consensus_pairs = _refuse

    def close(self):
        pass


def test_snp_diversity_consensus_exits_on_a_frequency_it_cannot_round(tmp_path):
    d = str(tmp_path / 'ragged')
    H._write_species(d, C.with_cell(H.VEC['species']['ragged'], 'freq', 7, 3, 'inf'))
    with pytest.raises(SystemExit) as e:
        H._run('snp_diversity.py', str(tmp_path), dict(species='ragged', options=['--consensus']), str(tmp_path / 'o'))
    assert e.value.code == C.ROUND_EXIT % (d, 8, 's002')
    # neither of the other two commands rounds a frequency or weights by depth: like the reference they go on
    H._run('snp_diversity.py', str(tmp_path), dict(species='ragged', options=[]), str(tmp_path / 'o'))
    H._run('call_consensus.py', str(tmp_path), dict(species='ragged', options=[]), str(tmp_path / 'o'))


@pytest.mark.parametrize("bad, text", [((3, 6, 2), C.ROUND_EXIT), ((6, 6, -1), C.ZERO_DEPTH_EXIT)])
def test_every_command_names_file_line_and_sample_of_a_refused_site(tmp_path, bad, text):
    d = str(tmp_path / 'ragged')
    H._write_species(d, H.VEC['species']['ragged'])
    message = text % ((d, 8, 's002') if bad[2] >= 0 else (d, 8))
    for script in ('snp_diversity.py', 'call_consensus.py'):
        with pytest.raises(SystemExit) as e:
            H._run(script, str(tmp_path), dict(species='ragged', options=[]), str(tmp_path / 'o'), make_context=lambda: _Refusing(bad))
        assert e.value.code == message
    with pytest.raises(SystemExit) as e:
        HT._run(d, [], str(tmp_path / 'o'), make_context=lambda: _Refusing(bad))
    assert e.value.code == message
