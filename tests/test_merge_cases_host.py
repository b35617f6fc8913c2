"""tests/merge_cases.py checked on the host: its vectorised model against oracle/merge_oracle.py looped site by site (on every
chosen table, on random sites, and up to the site where the oracle raises ZeroDivisionError), every case's claim under the model
alone, and what the tables laid over each kernel form must contain.  No device, no midas_amd."""
import functools

import numpy as np
import pytest

from oracle import merge_oracle as mo
from tests import merge_cases as MC

TABLE = MC.FORM_TABLE + MC.PREV_TABLE
IDS = ['S%d%s' % (S, '_deep' if deep else '') for S, deep in TABLE]


@functools.lru_cache(maxsize=None)
def groups(S, deep):
    return MC.groups(S, deep)


def oracle_loop(counts, mean, args):
    """The oracle over the sites in file order -> the arrays of Context.merge_sites, and 'raises': where prevalence() raised
    ZeroDivisionError (the loop ends there, as merge_midas.py would), else -1."""
    S, n = counts.shape[0], counts.shape[1]
    o = dict(major=np.full(n, 255, np.uint8), minor=np.full(n, 255, np.uint8), snp_type=np.zeros(n, np.uint8), flag=np.zeros(n, np.uint8),
             count_samples=np.zeros(n, np.uint32), pooled=np.zeros((n, 4), np.uint64), depth=np.zeros((S, n), np.uint32),
             minor_count=np.zeros((S, n), np.uint32), raises=-1)
    rows = np.ascontiguousarray(np.asarray(counts).transpose(1, 0, 2)).tolist()
    mean = [float(m) for m in mean]
    for i, c in enumerate(rows):
        pooled = mo.pooled_counts(c)
        major, minor, snp = mo.call_alleles(pooled, args['allele_freq'])
        _, depths = mo.per_sample(c, major, minor)
        try:
            cs, prev = mo.prevalence(mean, depths, args['site_depth'], args['site_ratio'])
        except ZeroDivisionError:
            o['raises'] = i
            break
        o['major'][i] = 255 if major is None else major
        o['minor'][i] = 255 if minor is None else minor
        o['snp_type'][i] = MC.SNP_NAMES.index(snp)
        o['flag'][i] = {None: 0, 'min_prev': 1, 'snp_type': 2}[mo.flag_reason(prev, snp, args['site_prev'], args['snp_type'])]
        o['count_samples'][i] = cs
        o['pooled'][i] = pooled
        o['depth'][:, i] = depths
        if minor is not None:
            o['minor_count'][:, i] = [x[minor] for x in c]
    return o


def same(got, exp, upto=None, what=''):
    assert got['raises'] == exp['raises'], what
    for k in MC.FIELDS:
        g, e = (got[k], exp[k]) if k not in ('depth', 'minor_count') else (got[k].T, exp[k].T)
        assert np.array_equal(g[:upto], e[:upto]), (what, k)


@pytest.mark.parametrize("S,deep", TABLE, ids=IDS)
def test_model_is_the_oracle_on_every_chosen_table(S, deep):
    for g in groups(S, deep):
        same(MC.model(g.counts, g.mean, g.args), oracle_loop(g.counts, g.mean, g.args), what=g.name)


VARIANTS = [dict(), dict(snp_type=['bi'], site_prev=0.95), dict(snp_type=['mono', 'tri', 'quad'], allele_freq=0.05, site_prev=0.6),
            dict(site_depth=15, site_ratio=1.1, site_prev=0.4, allele_freq=0.2), dict(site_depth=0, site_ratio=0.0, site_prev=0.2, snp_type=['bi', 'tri'])]


@pytest.mark.parametrize("S", sorted(set(S for S, _ in TABLE)) + [3])
def test_model_is_the_oracle_on_random_sites(S):
    """Shallow sites, sites with one large count, sites where every sample is large (the pooled sums pass 2^32)."""
    n = 2400
    rng = np.random.default_rng(900 + S)
    c = MC.random_sites(900 + S, S, n)
    edge = [255, 256, 65535, 65536, 2**28 - 1, 2**28, 2**31 - 1]
    for j, i in enumerate(range(0, n, 7)):
        c[(3 * j) % S, i, j % 4] = edge[j % len(edge)]
    c[:, 3::50, 1] = 2**31 - 1 - np.arange(S)[:, None]
    mean = (5.0 + 0.37 * (np.arange(S) % 64) + rng.random(S)).tolist()
    args = dict(MC.DEFAULTS, **VARIANTS[S % len(VARIANTS)])
    same(MC.model(c, mean, args), oracle_loop(c, mean, args))


@pytest.mark.parametrize("S", [1, 2, 9, 65, 130])
def test_model_raises_where_the_oracle_raises(S):
    for z, zero in zip(sorted({0, S // 2, S - 1}), (0.0, -0.0, 0.0)):
        for name, c, mean, args, first in MC.zero_mean_tables(S, z, zero, 300, [20, 90, 200, 290]):
            got, exp = MC.model(c, mean, args), oracle_loop(c, mean, args)
            assert got['raises'] == exp['raises'] == first, name
            same(got, exp, upto=first, what=name)
            if name.endswith('_big'):
                assert c[z, first].max() >= MC.BIG
    # no sample of mean zero: nothing raises, whatever the depth
    c = MC.random_sites(1, S, 50)
    assert MC.model(c, [10.0] * S, MC.DEFAULTS)['raises'] == -1


@pytest.mark.parametrize("S,deep", TABLE, ids=IDS)
def test_every_claim_holds_under_the_model(S, deep):
    n_claims = 0
    for g in groups(S, deep):
        out = MC.model(g.counts, g.mean, g.args)
        assert out['raises'] == -1
        for field, rows, expected in g.claims:
            assert out[field][rows].tolist() == list(expected), (g.name, field, rows)
            n_claims += 1
    assert n_claims > 100


@pytest.mark.parametrize("S,deep", TABLE, ids=IDS)
def test_a_border_row_differs_from_a_neighbour(S, deep):
    """allele_freq: below / on / above name types r, r + 1, r + 1 for every rank r that can reach the literal; prevalence: k - 1
    passing samples flag the site and k + 1 keep it, and k decides between site_prev = k / S and the next double above it."""
    seen_ranks = set()
    for g in groups(S, deep):
        out = MC.model(g.counts, g.mean, g.args)
        if g.name.startswith('allele_freq_0.') or g.name == 'allele_freq_1':
            for field, rows, expected in g.claims:
                t = out['snp_type'][rows].tolist()
                assert t[0] + 1 == t[1] and (len(t) < 3 or t[2] == t[1]), (g.name, rows)
                seen_ranks.add((g.name, t[1]))
        if g.name.startswith('prev_'):
            for field, rows, expected in g.claims:
                if field == 'flag' and len(rows) == 3:
                    f = out['flag'][rows].tolist()
                    assert f[0] == 1 and f[2] == 0 and f[1] in (0, 1)
    # the ranks that can sit on each literal: the major allele holds at least a quarter, so 0.01, 0.05 and 0.2 take ranks 1..3;
    # 1/3 ranks 0..2, 0.5 ranks 0 and 1, 1.0 the major allele alone
    assert len(seen_ranks) == 3 + 3 + 3 + 3 + 2 + 1
    exact = [g for g in groups(S, deep) if g.name.startswith('prev_') and g.marks['exact_prev']]
    assert exact, "no site_prev that k / S hits exactly"
    up = [g for g in groups(S, deep) if g.name.startswith('prev_') and not g.marks['exact_prev']]
    flags = [[e for f, r, e in g.claims if f == 'flag'][0] for g in up]
    assert [1, 0, 0][:len(flags[0])] in flags and [1, 1, 0][:len(flags[0])] in flags


@pytest.mark.parametrize("S,deep", TABLE, ids=IDS)
def test_what_the_table_of_every_form_contains(S, deep):
    types, flags, ties = set(), set(), set()
    fallback = exact_freq = exact_prev = 0
    for g in groups(S, deep):
        out = MC.model(g.counts, g.mean, g.args)
        types |= set(out['snp_type'].tolist())
        flags |= set(out['flag'].tolist())
        for r in g.marks.get('fallback', []):
            assert g.counts[:, r].max() >= MC.BIG
            fallback += 1
        pooled = g.counts.sum(axis=0)
        for kind, rows in g.marks.items():
            if kind.startswith('tie_'):
                for r in rows:
                    p = sorted(pooled[r].tolist())
                    assert len(set(p)) < 4 or kind == 'tie_depth_zero'
                ties.add(kind)
        for r in g.marks.get('exact_freq', []):
            f = np.sort(pooled[r] / pooled[r].sum())
            assert (f == g.args['allele_freq']).any()
            exact_freq += 1
        for r in g.marks.get('exact_prev', []):
            assert out['count_samples'][r] / float(S) == g.args['site_prev'] and out['flag'][r] == 0
            exact_prev += 1
    assert types == {0, 1, 2, 3, 4} and flags == {0, 1, 2}
    assert ties == {'tie_' + k for k in MC.TIE_SETS}
    assert fallback and exact_freq and exact_prev
    form = MC.form_of(S, groups(S, deep)[0].mean)
    assert form == MC.form_of(S, groups(S, deep)[-1].mean)
    z = MC.zero_positions(S, form)[-1]
    name, c, mean, args, first = MC.zero_mean_tables(S, z, 0.0, 40, [20, 30], deep)[0]
    assert MC.model(c, mean, args)['raises'] == first == 20 and MC.form_of(S, mean) == form


def test_every_form_meets_a_prevalence_that_only_the_double_division_gets_right():
    """k / S == site_prev at 0.5 or 1.0 is exact in any arithmetic.  3/5 == 0.6 and 19/20 == 0.95 hold for the reference's double
    division; every form gets such a row (kept on it, flagged one sample below), and one at which k * (1.0 / S) is another
    double than k / S, so that a kernel multiplying by the reciprocal would flag the site."""
    exact, told_apart = {}, set()
    for S, deep in TABLE:
        for g in groups(S, deep):
            p = g.args['site_prev']
            if not (g.name.startswith('prev_') and g.marks['exact_prev']) or p in (0.5, 1.0):
                continue
            form = MC.form_of(S, g.mean)
            form = form if form.startswith('split') else form.split(' ')[0]
            out = MC.model(g.counts, g.mean, g.args)
            for r in g.marks['exact_prev']:
                k = int(out['count_samples'][r])
                assert k / float(S) == p and out['flag'][r] == 0 and out['flag'][r - 1] == 1, (S, p)
                if k * (1.0 / S) != p:
                    told_apart.add(form)
            exact.setdefault(form, set()).add((S, p))
    assert set(exact) == told_apart == {'regs32', 'regs16', 'bytes', 'split G=8', 'split G=16'}, (exact, told_apart)
    assert (5, 0.6) in exact['regs32'] and {(20, 0.95), (40, 0.95), (60, 0.95)} <= exact['regs16'] and (100, 0.95) in exact['bytes']


def test_forms():
    f = MC.form_of
    assert [f(S, [10.0] * S) for S in (1, 8, 9, 64)] == ['regs32', 'regs32', 'regs16', 'regs16']
    assert [f(S, [64.0] * S) for S in (65, 72, 73, 128)] == ['bytes S=72', 'bytes S=72', 'bytes S=80', 'bytes S=128']
    assert [f(S, [64.0] * (S - 1) + [MC.DEEP]) for S in (65, 111, 112, 128)] == ['split G=8', 'split G=8', 'split G=16', 'split G=16']
    assert [f(S, [1.0] * S) for S in (129, 200)] == ['split G=16', 'split G=16']
    assert f(64, [1e300] * 64) == 'regs16'
    covered = {f(S, groups(S, deep)[0].mean).split('=')[0] for S, deep in MC.FORM_TABLE}
    assert covered == {'regs32', 'regs16', 'bytes S', 'split G'}
    # one mean of DEEP among means of 64 changes no sample's limits at site_ratio 2: the two forms then see the same problem
    assert MC.limits(64.0, 2.0, 1) == MC.limits(MC.DEEP, 2.0, 1) == (1, 128)
