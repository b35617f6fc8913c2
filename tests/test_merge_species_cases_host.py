"""tests/merge_species_cases.py without a device: the model (tests/merge_species_model.py) runs every case -- the accepted ones
without raising, the refused ones raising the stated reason on the stated line of the stated sample -- and every case sits on
what it says it sits on: sums that depend on numpy's order of additions, the LDS or long-row form implied by (S, lds_bound),
designed middles, halves under round(x, 2), prevalence 0 and S with the order key's top bit, probe chains of the stated shape,
all sixteen residues of the fields kernel's words, more row blocks than one wave of the writer."""
import math

import numpy as np
import pytest

from tests import merge_species_cases as K
from tests import merge_species_model as M

ALL = [n for f in K.FAMILIES for n in K.names(f)]


def bits(x):
    return np.asarray(x, np.float64).view(np.uint64).tolist()


@pytest.mark.filterwarnings("ignore:overflow encountered")
@pytest.mark.parametrize("name", ALL)
def test_the_model_runs_every_case(name):
    c = K.named(name)
    assert len(c['sample_ids']) == len(c['profiles']) > 0 and len(set(c['ids'])) == len(c['ids']) and c['on']
    want = K.expect(c)
    if c['refused']:
        assert isinstance(want, M.BadProfile), name
    else:
        assert set(want['files']) == set(M.FILES) and len(want['coverage']) == len(c['ids']) and len(want['coverage'][0]) == len(c['profiles'])
        assert sorted(want['order']) == list(range(len(c['ids'])))
    for kw, lds in c['forms']:
        assert set(kw) <= {'chunk_bytes', 'lds_bound'}
        assert lds is None or c['refused'] or lds == K.lds_form(len(c['profiles']), kw.get('lds_bound', 0)), (name, kw)


def test_every_family_is_there():
    assert [c['name'].split('/')[1] for c in K.cases('rows')] == [str(S) for S in (511, 512, 513, 1000, 1024, 1025, 2049, 4090, 4096)]
    assert [c['name'] for c in K.cases('rowsof')] == ['rowsof/%d' % S for S in (1, 2, 3, 4, 8, 9, 16, 17)]
    assert len(K.cases('prev')) == 6 * 5 and len(K.cases('switch')) == 8 and len(set(ALL)) == len(ALL)
    forms = dict((c['name'], [(len(c['profiles']), kw.get('lds_bound', 0), lds) for kw, lds in c['forms']]) for c in K.cases('switch'))
    assert forms['switch/default_4096'][0] == (4096, 0, True) and forms['switch/default_4097'] == [(4097, 0, False)]
    assert forms['switch/bound_S_and_S-1'] == [(9, 9, True), (9, 8, False)]
    assert [(len(c['ids']), len(c['profiles']), c['row_bits']) for c in K.cases('switch')[3:]] == [(1, 2, 1), (2, 3, 1), (3, 2, 2), (4, 5, 2), (5, 4, 3)]
    for c in K.cases('switch')[3:]:
        assert c['forms'] == [(dict(lds_bound=1), False), ({}, True)]
    for f in ('rowsof', 'prev'):
        for c in K.cases(f):                                                   # both forms wherever a row has two samples
            assert [lds for _, lds in c['forms']] == ([True, False] if len(c['profiles']) > 1 else [True])


@pytest.mark.parametrize("name", K.names('rows') + ['switch/default_4097'])
def test_long_rows_depend_on_the_order_of_the_additions(name):
    c = K.named(name)
    S = len(c['profiles'])
    assert K.cut_matters(S) == (S in (511, 1000, 4090))
    for m in ('cov_texts', 'ab_texts'):
        assert any(K.order_sensitive(row) for row in c[m]), (name, m)
        texts = [v for row in c[m] for v in row]
        assert any(v.startswith('-') for v in texts) and any(len(v.lstrip('-').replace('.', '').lstrip('0').split('e')[0]) >= 17 for v in texts)
    want = K.expect(c)                                                         # the rows the model sums are the rows asserted on
    assert bits(want['mean_coverage']) == bits([np.add.reduce(np.array([float(v) for v in row])) / S for row in c['cov_texts']])


def test_the_pairwise_sums_written_out_here_are_numpys():
    rng = np.random.default_rng(5)
    for n in (1, 7, 8, 9, 127, 128, 129, 255, 511, 1000, 4097):
        a = [float(v) for v in K.mixed_values(rng, n)]
        assert bits(K.halving_sum(a, True)) == bits(0.0 + np.add.reduce(np.array(a))), n
    assert [K.cut_matters(n) for n in (128, 129, 255, 256, 257, 272, 496, 4096, 4097, 4100)] == [False, False, True, False, False, True, True, False, False, True]


@pytest.mark.filterwarnings("ignore:overflow encountered")
@pytest.mark.parametrize("S", K.DESIGNED_S)
def test_designed_rows_are_what_they_say(S):
    c = K.named('rowsof/%d' % S)
    rows = dict(zip(c['designed'], c['cov_texts']))
    assert len(rows) == 12
    val = dict((w, sorted(float(v) for v in r)) for w, r in rows.items())
    lo, hi = (S - 1) // 2, S // 2
    pick = lambda word: [w for w in rows if word in w][0]
    assert len(set(rows[pick('all values equal')])) == 1
    assert set(rows[pick('all -0.0')]) == {'-0.0'}
    for w in (pick('-0.0 and 0.0 around'), pick('0.0 below -0.0')):
        assert set(rows[w]) == {'-0.0', '0.0'} or (S == 1 and len(set(rows[w]) & {'-0.0', '0.0'}) == 1)
    assert val[pick('all negative')][-1] < 0
    if S > 1:
        assert val[pick('straddles')][lo] < 0 < val[pick('straddles')][hi] or S % 2
        assert val[pick('straddles')][0] < 0 < val[pick('straddles')][-1]
    if S > 2:
        t = val[pick('ties')]
        assert t[lo] == t[hi] == t[min(hi + 1, S - 1)] and (S < 4 or t[lo - 1] == t[lo]) and (S < 8 or len(set(t)) == 3)
    if S % 2 == 0:
        a, b = val[pick('inexact')][lo], val[pick('inexact')][hi]
        assert (a, b) == (1.0, float(np.nextafter(1.0, 2.0))) and a + b == 2.0          # 2.0000000000000002 is no double: the sum is rounded
        assert val[pick('overflows')][lo:hi + 1] == [1e308, 1.7e308] and math.isinf(1e308 + 1.7e308)
    words = lambda w: (set(x >> 32 for x in bits(val[w])), set(x & 0xFFFFFFFF for x in bits(val[w])))
    high, low = words(pick('low word only'))
    assert len(high) == 1 and len(low) == min(S, 3)
    high, low = words(pick('high word only'))
    assert len(low) == 1 and len(high) == min(S, 7)
    assert all(abs(v) < 2.3e-308 for v in val[pick('subnormals')]) and 5e-324 in val[pick('subnormals')]
    want = K.expect(c)
    # every designed row is a coverage row of one species and the abundance row of the species in front of it
    for g in range(12):
        assert sorted(bits(want['abundance'][g])) == sorted(bits(want['coverage'][(g + 1) % 12]))
    if S >= 8:
        g = c['designed'].index(pick('all -0.0'))
        assert bits(want['mean_coverage'][g]) == bits(0.0) != bits(-0.0)                  # numpy starts from 0.0: the sum of -0.0s is 0.0


@pytest.mark.filterwarnings("ignore:overflow encountered")
def test_rounding_values_lie_on_halves():
    c = K.named('round/halves')
    assert [row.split('\t')[2] for row in c['profiles'][0].split('\n')[1:-1]] == K.ROUND_VALUES
    assert K.ROUND_VALUES == ['0.125', '0.375', '2.675', '1.005', '0.005', '-0.005', '-0.004', '0.285', '1e307', '123456.785', '0.0', '-0.0']
    for text in K.ROUND_VALUES:
        v = np.float64(text)
        assert bits(round(v, 2)) == bits(np.rint(v * 100.0) / 100.0), text
    want = K.expect(c)
    assert bits(want['mean_coverage']) == bits(want['median_coverage']) == bits([0.0 + float(v) for v in K.ROUND_VALUES])      # (numpy starts from 0.0: -0.0 alone is 0.0)
    assert bits(want['rounded']['mean_coverage']) == bits([round(np.float64(0.0) + np.float64(v), 2) for v in K.ROUND_VALUES])
    cells = [line.split('\t') for line in want['files']['species_prevalence.txt'].split('\n')[1:-1]]
    assert any(x[1] == '-0.0' for x in cells) and any(x[1] == 'inf' for x in cells) and any(x[3] == '-0.0' for x in cells) and any(x[3] == 'inf' for x in cells)
    assert str(round(np.float64(0.125), 2)) == '0.12' and str(round(np.float64(0.375), 2)) == '0.38' and str(round(np.float64(2.675), 2)) == '2.68' != str(round(2.675, 2))


@pytest.mark.parametrize("name", K.names('prev'))
def test_prevalence_cases_hold_both_ends_and_ties(name):
    c = K.named(name)
    S, depth, want = len(c['profiles']), c['sample_depth'], K.expect(c)
    assert want['prevalence'] == c['counts']
    stable = sorted(range(len(c['ids'])), key=lambda k: (-want['prevalence'][k], k))
    assert want['order'] == stable and want['order'] != list(range(len(c['ids']))) or math.isinf(depth)
    values = set(v for row in want['coverage'] for v in row)
    if math.isinf(depth):
        assert set(want['prevalence']) == {0} and max(values) == 1.7976931348623157e308
        return
    assert 0 in want['prevalence'] and S in want['prevalence']
    assert len(want['prevalence']) - len(set(want['prevalence'])) >= 4                   # ties at both ends and in between
    assert values == {depth, float(np.nextafter(np.float64(depth), -np.inf))}
    if depth == 0.0 and S > 1:
        assert any(math.copysign(1.0, v) < 0 and v == 0.0 for row in want['coverage'] for v in row)      # -0.0 >= 0.0 counts
    if S & (S - 1) == 0:
        s_bits = 1
        while (1 << s_bits) <= S:
            s_bits += 1
        assert (S - 0) >> (s_bits - 1) == 1                                              # prevalence 0: the key S needs the top bit


def test_prevalence_cases_cover_every_depth_at_every_size():
    assert set((len(c['profiles']), c['sample_depth']) for c in K.cases('prev')) == set((S, d) for S in (1, 2, 4, 8, 128, 256) for d in (0.0, 0.5, 1.0, -2.5, math.inf))


def test_lookup_chains_have_the_stated_shape():
    t = dict((c['name'].split('/')[1], c) for c in K.cases('table'))
    one = t['seven_in_one_slot']
    assert len(one['ids']) == 7 and K.table_of(one['ids'])[0] == 16 and set(K.home(s, 16) for s in one['ids']) == {4}
    assert K.table_of(one['ids'])[2] == one['chain'] == [4, 5, 6, 7, 8, 9, 10]
    assert [len(K.probe(one['ids'], s)[0]) for s in one['ids']] == [1, 2, 3, 4, 5, 6, 7]
    wrap = t['wraps_to_slot_0']
    assert K.table_of(wrap['ids'])[2] == wrap['chain'] and wrap['chain'][:4] == [15, 0, 1, 2]
    assert [K.home(s, 16) for s in wrap['ids'][:4]] == [15, 15, 15, 0] and K.probe(wrap['ids'], wrap['ids'][2])[0] == [15, 0, 1]
    for name in ('refused_head_of_the_full_chain', 'refused_in_the_wrapped_chain'):
        c = t[name]
        assert K.probe(c['ids'], c['intruder']) == (c['visits'], None) and c['intruder'] not in c['ids']
    assert len(t['refused_head_of_the_full_chain']['visits']) == 8 and t['refused_in_the_wrapped_chain']['visits'] == [15, 0, 1, 2, 3]
    assert [(R, t['%d_ids' % R]['size'], K.table_of(t['%d_ids' % R]['ids'])[0]) for R in (7, 8, 15, 16)] == [(7, 16, 16), (8, 32, 32), (15, 32, 32), (16, 64, 64)]
    for R in (7, 8, 15, 16):
        assert len(t['%d_ids' % R]['ids']) == R and max(K.raw(t['%d_ids' % R]['ids'][0])) > 0x7F
    for kind in ('last_byte', 'first_byte', 'prefix', 'extension', 'empty'):
        c = t['refused_' + kind]
        known, intruder = c['near'], c['intruder']
        size = K.table_size(len(c['ids']))
        visits, found = K.probe(c['ids'], intruder)
        assert found is None and known in c['ids'] and intruder not in c['ids']
        if kind == 'last_byte':
            assert len(known) == len(intruder) and known[:-1] == intruder[:-1] and K.home(known, size) == K.home(intruder, size) and len(visits) >= 2
        elif kind == 'first_byte':
            assert len(known) == len(intruder) and known[1:] == intruder[1:] and K.home(known, size) == K.home(intruder, size) and len(visits) >= 2
        elif kind == 'prefix':
            assert known.startswith(intruder) and 0 < len(intruder) < len(known) and len(visits) >= 2
        elif kind == 'extension':
            assert intruder.startswith(known) and len(intruder) == len(known) + 1 and len(visits) >= 2
        else:
            assert intruder == ''
    for c in K.cases('table'):
        want = K.expect(c)
        if c['refused']:
            line = 1 + [x.split('\t')[0] for x in c['profiles'][1].split('\n')].index(c['intruder'])
            assert (want.reason, want.sample, want.line, want.what) == (M.UNKNOWN, 1, line, c['intruder']) and line >= 2


def test_the_fields_case_covers_all_sixteen_residues():
    c = K.named('fields/sixteen_residues')
    p0, p1 = c['profiles']
    every = set(range(16))
    # sample 0 stands at offset 0 of its group at either chunk size; sample 1 behind it in one group, at offset 0 in a group of its own
    for text, offset in ((p0, 0), (p1, 0), (p1, len(p0.encode()) + 1)):
        got = K.residues(text, offset)
        assert set(got) == {'start', 'end'} | set(M.COLUMNS)
        for what, seen in got.items():
            assert seen == every, (what, offset, sorted(every - seen))
    first = [len(line.split('\t')[0]) for line in p0.split('\n')[1:-1]]
    assert set(range(16)) <= set(first) and max(first) > 16 and p0.split('\n')[0].split('\t') == ['note'] + list(M.COLUMNS) + ['tail']


def test_field_cases_are_what_they_say():
    t = dict((c['name'].split('/')[1], c) for c in K.cases('fields'))
    for c in t.values():
        assert c['forms'] == [(dict(chunk_bytes=0), True), (dict(chunk_bytes=16), True)] and len(c['profiles']) >= 2
    h0, h1 = [p.split('\n')[0].split('\t') for p in t['forty_columns']['profiles']]
    assert len(h0) == len(h1) == 40 and [h0.index(n) for n in M.COLUMNS] == [0, 17, 38, 39] and [h1.index(n) for n in M.COLUMNS] == [39, 38, 17, 0]
    assert any('\t\t' in line for line in t['forty_columns']['profiles'][0].split('\n')[1:])                       # an empty cell
    assert len(t['forty_columns']['profiles'][0].split('\n')[1]) > 5 * 16
    lines = t['dropped_lines']['profiles'][1].split('\n')
    assert sorted(len(x.split('\t')) for x in lines[:-1]) == [3, 3, 4, 4, 4, 4, 5, 5] and '\t\t' in lines and '\t\t\t\t' in lines
    assert K.expect(t['dropped_lines'])['files'] == M.merge(K.sample_names(3), [K.GOOD] * 3, K.GOOD_IDS, 1.0)['files']
    want = K.expect(t['int64_ends'])
    assert want['reads'][0][1] == 2 ** 63 - 1 and want['reads'][1][1] == -2 ** 63
    assert not t['no_final_newline']['profiles'][1].endswith('\n') and K.expect(t['no_final_newline'])['coverage'][2] == [0.0, 0.0, 0.0]
    crlf = t['crlf_unnamed_last']['profiles'][1]
    assert crlf.count('\r\n') == crlf.count('\n') == 4 and crlf.split('\r\n')[0].split('\t')[-1] == 'z'
    assert K.expect(t['crlf_unnamed_last'])['files'] == K.expect(t['no_final_newline'])['files']
    look = t['lookalike_headers']['profiles'][1].split('\n')
    assert look[0].split('\t') == ['coverage2', ' species_id', 'Coverage'] + list(M.COLUMNS) and look[1].split('\t')[:3] == ['9.5', 'q', '8.5']
    assert K.expect(t['lookalike_headers'])['files'] == K.expect(t['no_final_newline'])['files']
    stated = dict(empty_count_reads=(7, 3), empty_coverage=(8, 3), count_reads_plus=(7, 4), count_reads_minus=(7, 4), **{'count_reads_1.0': (7, 4)},
                  crlf_named_last=(4, 1), coverage2_for_coverage=(3, 1), blank_species_id=(1, 1), Coverage_for_coverage=(3, 1))
    for name, (reason, line) in stated.items():
        c = t['refused_' + name]
        want = K.expect(c)
        assert (want.reason, want.sample, want.line) == (reason, 1, line) == (c['reason'], 1, line), name
    alone = t['refused_header_alone']
    want = K.expect(alone)
    assert alone['profiles'][1] == 'species_id\tcount_reads\tcoverage\trelative_abundance' and (want.reason, want.sample, want.what) == (M.MISSING, 1, 'a')
    assert len([c for c in t.values() if c['refused']]) == 10


def test_the_writer_case_needs_a_second_wave():
    c = K.named('write/five_blocks')
    R, S = len(c['ids']), len(c['profiles'])
    block = 65536 // S
    assert R * S > 4 * 65536 and R > 4 * block and c['blocks'] == -(-R // block) == 5 and c['write_threads'] == (1, 2)
    assert 4 * 1 < c['blocks'] <= 4 * 2                                            # two waves of one thread, one wave of two
    assert all(p.split('\n', 2)[1].startswith(c['ids'][0] + '\t') for p in c['profiles'][:50])      # shuffle=False: rows in the ids' order
