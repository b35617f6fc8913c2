"""Chosen tables for the per-site kernels (sites_rows.h, sites_call.h, sites_scan.hip, sites_strains.hip): every case puts rows or samples ON a decision of the site loop and
one step to either side of it, where random tables almost never land.  Plain data and the searches that find it -- nothing
here knows the kernels.  tests/test_site_cases_host.py asserts with the sequential model alone that every case sits where its
name says; tests/test_gpu_site_borders.py holds the device to the model on them, bit for bit.

A case is (name, frows, drows, mask, cols, mean, opts, note): the cell strings of the two matrices by row, the site mask, the
matrix columns in use, their mean depths, the keyword arguments of sites_scan, and what the host check asserts about it."""
import collections
import math
from fractions import Fraction

import numpy as np

WEIGHT, ROUND, POOLED, PER_GENE, MASK_ONLY, SEQ, SUMS = 1, 2, 4, 8, 16, 32, 64      # abi.SITES_* (the host check compares them)
INF = float('inf')
MINOR, MAJOR = ord('a'), ord('b')

Case = collections.namedtuple('Case', 'name frows drows mask cols mean opts note')
DEFAULTS = dict(site_depth=1, site_ratio=INF, allele_support=0.0, site_prev=0.0, site_maf=0.0, snp_maf=0.01, max_sites=-1, flags=SUMS)


def up(x, k=1):
    for _ in range(k):
        x = math.nextafter(x, INF)
    return x


def down(x, k=1):
    for _ in range(k):
        x = math.nextafter(x, -INF)
    return x


def bits(x):
    return np.float64(x).view(np.uint64)


def matrix(cells_by_row, eol='\n'):
    return np.frombuffer(''.join('%d\t%s%s' % (r + 1, '\t'.join(row), eol) for r, row in enumerate(cells_by_row)).encode(), np.uint8)


def case(name, frows, drows, mean=None, mask=None, cols=None, note=None, groups=(), **opts):
    """groups: (group_rows, chunk_bytes) settings to run besides the usual ones, where a border must fall on a chosen row."""
    n_cols = len(frows[0])
    cols = list(range(n_cols)) if cols is None else list(cols)
    o = dict(DEFAULTS)
    o.update(opts)
    return Case(name, frows, drows, np.ones(len(frows), np.uint8) if mask is None else np.asarray(mask, np.uint8), cols,
                [10.0] * len(cols) if mean is None else [float(x) for x in mean], o, dict(note or {}, groups=tuple(groups)))


def run(scan, c, rows=None, **over):
    """scan (the model's sites_scan or the device's) on the case, or on some of its rows as a table of their own, with dumps."""
    pick = list(range(len(c.frows))) if rows is None else list(rows)
    opts = dict(c.opts)
    if 'site_gene' in opts:
        opts['site_gene'] = np.asarray(opts['site_gene'])[pick]
    opts.update(over)
    n = len(pick)
    return scan(matrix([c.frows[r] for r in pick]), matrix([c.drows[r] for r in pick]), c.mask[pick], c.cols, c.mean, dump=True,
                minor=np.full(n, MINOR, np.uint8), major=np.full(n, MAJOR, np.uint8), **opts)


def one_row(name, cells, note=None, **kw):
    """One site; cells = [(freq cell, depth cell)] by sample."""
    return case(name, [[f for f, _ in cells]], [[d for _, d in cells]], note=note, **kw)


# ---- sample decisions: depth, ratio, allele support ---------------------------------------------------------------------------------
def depth_cases():
    out = []
    for sd in (0, 1):
        ds = [sd - 1, sd, sd + 1, -3]
        out.append(one_row('depth_%d' % sd, [('0.25', str(d)) for d in ds], site_depth=sd, note=dict(kept=[False, True, True, False])))
    return out


def ratio_search(ratio, want):
    """-> (d, mean): d / mean is `ratio` itself ('on') or its fp64 neighbour above / below ('over' / 'under'), for a small d."""
    target = dict(on=ratio, over=up(ratio), under=down(ratio))[want]
    for d in range(1, 60):
        m0 = d / ratio
        for k in range(-4, 5):
            mean = up(m0, k) if k >= 0 else down(m0, -k)
            if d / mean == target:
                return d, mean
    raise AssertionError((ratio, want))


def ratio_cases():
    out = []
    for ratio, fixed in ((2.0, (5, 2.5)), (3.0, (7, 7 / 3.)), (0.7, None)):
        picks = [('on', fixed or ratio_search(ratio, 'on')), ('over', ratio_search(ratio, 'over')), ('under', ratio_search(ratio, 'under'))]
        out.append(one_row('ratio_%g' % ratio, [('0.25', str(d)) for _, (d, _) in picks], mean=[m for _, (_, m) in picks], site_ratio=ratio,
                           note=dict(kept=[True, False, True], ratio=[(d, m, w) for w, (d, m) in picks])))
    out.append(one_row('ratio_zero', [('0.25', '0'), ('0.25', '1'), ('0.25', '-1')], site_ratio=0.0, site_depth=-5, note=dict(kept=[True, False, True])))
    out.append(one_row('ratio_inf', [('0.25', '1'), ('0.25', '999999999999999999'), ('0.25', '1152921504606846977')], site_ratio=INF,
                       mean=[1e-300, 1e-300, 1e-300], note=dict(kept=[True, True, True])))
    out.append(one_row('ratio_negative', [('0.25', '0'), ('0.25', '-3'), ('0.25', '-2'), ('0.25', '-1')], site_ratio=-1.0, site_depth=-10,
                       mean=[2.0] * 4, note=dict(kept=[False, True, True, False])))
    # float(depth) rounds: 2^53 + 1 is 2^53 as a double, and so not above a ratio of 2^53; the 19-digit cell is the host's
    p53 = 1 << 53
    out.append(one_row('ratio_2p53', [('0.25', str(p53 - 1)), ('0.25', str(p53)), ('0.25', str(p53 + 1)), ('0.25', str(p53 + 2)), ('0.25', str(p53 + 3)),
                                      ('0.25', '18014398509481985'), ('0.25', '1152921504606846977')],
                       site_ratio=float(p53), mean=[1.0] * 7, note=dict(kept=[True, True, True, False, False, False, False])))
    return out


def support_cases():
    out = []
    out.append(one_row('support_0.55', [(f, '5') for f in ('0.55', '0.54999999999999993', '0.5500000000000002', '0.45', '0.44999999999999996',
                                                           '0.45000000000000007', '0.4499999999999999', '0.5')], allele_support=0.55,
                       note=dict(kept=[True, False, True, True, True, False, True, False], f_on=['0.55'], q_on=['0.45'])))
    out.append(one_row('support_0.5', [(f, '5') for f in ('0.5', '0.49999999999999994', '0.5000000000000001', '0', '1', '-0.0', '1.0000000000000002')],
                       allele_support=0.5, note=dict(kept=[True] * 7, f_on=['0.5'], q_on=['0.5'])))
    out.append(one_row('support_just_above_0.5', [(f, '5') for f in ('0.5', '0.49999999999999994', '0.5000000000000001', '0.49999999999999989')],
                       allele_support=up(0.5), note=dict(kept=[False, False, True, True], f_on=['0.5000000000000001'], q_on=['0.49999999999999989'])))
    out.append(one_row('support_1', [(f, '5') for f in ('0', '1', '-0.0', '1.0000000000000002', '0.9999999999999999', '1e-17', '1.2e-16', '-1e-300')],
                       allele_support=1.0, note=dict(kept=[True, True, True, True, False, True, False, True], f_on=['1'], q_on=['0', '-0.0', '1e-17'])))
    out.append(one_row('support_0', [(f, '5') for f in ('0', '1', '-0.0', '1.0000000000000002', '0.5', '-3.5')], allele_support=0.0,
                       note=dict(kept=[True] * 6)))
    return out


# ---- site decisions: prevalence, pooled frequency --------------------------------------------------------------------------------
def _prev_rows(S, counts):
    """A row a count: that many samples with depth 1 (kept), at shifting places, the others with depth 0."""
    drows = []
    for r, c in enumerate(counts):
        on = set(sorted(range(S), key=lambda s: (s * 7 + r * 3) % S)[:c])
        drows.append(['1' if s in on else '0' for s in range(S)])
    return [['0.25'] * S for _ in counts], drows


def prevalence_cases():
    out = []
    for S, k, prev in ((10, 3, '0.3'), (3, 1, '0.3333333333333333'), (3, 2, '0.6666666666666666')) + tuple((7, k, repr(k / 7)) for k in range(1, 7)):
        counts = [k - 1, k, k + 1]
        frows, drows = _prev_rows(S, counts)
        out.append(case('prev_%d_of_%d' % (k, S), frows, drows, site_prev=float(prev), flags=SUMS | POOLED,
                        note=dict(site_keep=[False, True, True], counts=counts, on=(k, S, float(prev)))))
    for prev in (1e-7, 1e-6):
        frows, drows = _prev_rows(10, [0, 1])
        out.append(case('prev_floor_%g' % prev, frows, drows, site_prev=prev, flags=SUMS | POOLED, note=dict(site_keep=[False, True], counts=[0, 1])))
    frows, drows = _prev_rows(10, [0, 1])
    out.append(case('prev_off', frows, drows, site_prev=0.0, flags=SUMS | POOLED, note=dict(site_keep=[True, True], counts=[0, 1], pooled0=[0])))
    return out


def pool_search(weights, site_maf, want):
    """-> three frequency cells whose (weighted) mean is site_maf ('on') or its neighbour ('over' / 'under')."""
    target = dict(on=site_maf, over=up(site_maf), under=down(site_maf))[want]
    for a in range(1, 40):
        for b in range(1, 40):
            f1, f2 = a / 64. + 0.003, b / 128. + 0.0007
            guess = (site_maf * sum(weights) - weights[0] * f1 - weights[1] * f2) / weights[2]
            for k in range(-6, 7):
                f3 = up(guess, k) if k >= 0 else down(guess, -k)
                if weights == [1, 1, 1]:
                    got = ((0.0 + f1 + f2) + f3) / 3
                else:
                    got = ((0.0 + weights[0] * f1) + weights[1] * f2 + weights[2] * f3) / sum(weights)
                if got == target and 0 < f3 < 1:
                    return [repr(f1), repr(f2), repr(f3)]
    raise AssertionError((weights, site_maf, want))


def pooled_cases():
    out = []
    maf = 0.25              # (three values never average to 0.2 itself: 0.6 / 3 and the next double / 3 round to either side of it)
    for name, w, flags in (('pooled_maf_unweighted', [1, 1, 1], SUMS | POOLED), ('pooled_maf_weighted', [1, 2, 3], SUMS | POOLED | WEIGHT)):
        wants = ['on', 'over', 'under']
        frows = [pool_search(w, maf, want) for want in wants] + [['0.9', '0.9', '0.9']]
        drows = [[str(x) for x in w] for _ in wants] + [['0', '0', '0']]
        out.append(case(name, frows, drows, site_maf=maf, flags=flags, note=dict(site_keep=[True, True, False, False], pool=(maf, wants), pooled0=[3])))
    out.append(case('pooled_maf_single', [['0.1'], ['0.09999999999999999'], ['0.10000000000000002']], [['4']] * 3, site_maf=0.1, flags=SUMS | POOLED,
                    note=dict(site_keep=[True, False, True])))
    return out


# ---- the unweighted pool: numpy's pairwise reduce at every change of its shape ------------------------------------------------------
PAIRWISE_COUNTS = (1, 7, 8, 9, 15, 16, 17, 127, 128, 129, 136, 255, 256, 257, 264, 300)


def sequential_sum(a):
    res = 0.0
    for x in a:
        res += x
    return res


def _pairwise_row(K, seed, row, pairwise_sum):
    """K kept samples among K + 3..10 columns: the dropped ones (depth 0) in front of, between and behind the kept ones."""
    rng = np.random.default_rng(seed)
    n_drop = 3 + (K + row) % 8
    S = K + n_drop
    drop = set(rng.choice(S, n_drop, replace=False).tolist())
    if row == 0:
        drop = set(range(n_drop))                       # all in front
    elif row == 1:
        drop = set(range(S - n_drop, S))                # all behind
    vals = 10.0 ** rng.uniform(-5, 0, S)
    f = ['%.17g' % v for v in vals]
    d = ['0' if s in drop else '3' for s in range(S)]
    kept = [float(f[s]) for s in range(S) if s not in drop]
    differs = bits(pairwise_sum(kept)) != bits(sequential_sum(kept))
    return f, d, differs


def pairwise_cases(pairwise_sum):
    """pairwise_sum: the model's (the host check passes it in).  Seeds are searched so that, from 8 values on, the pairwise
    and the left-to-right sums of every row differ in bits."""
    out = []
    for K in PAIRWISE_COUNTS:
        rows = []
        for row in range(3):
            seed = 1000 * K + 10 * row
            while True:
                f, d, differs = _pairwise_row(K, seed, row, pairwise_sum)
                if differs or K < 8:
                    break
                seed += 1
            rows.append((f, d))
        S = max(len(f) for f, _ in rows)
        frows = [f + ['0.5'] * (S - len(f)) for f, _ in rows]
        drows = [d + ['0'] * (S - len(d)) for _, d in rows]
        for tag, flags in (('', SUMS | POOLED), ('_round', SUMS | POOLED | ROUND)):
            out.append(case('pairwise_%d%s' % (K, tag), frows, drows, flags=flags, note=dict(pairwise=K)))
    return out


def weighted_cases():
    out = []
    frows = [['0.1', '0.7', '0.3', '0.9', '0.123456789'], ['0.3', '0.3', '0.3', '0.3', '0.3'], ['-0.0', '-0.0', '-0.0', '-0.0', '-0.0'],
             ['0.2', '0.6', '0.1', '0.4', '0.7']]
    drows = [['1', '1000000', '999999999999', '3', '77777'], ['3', '100000000000000000', '1', '7', '11'], ['1', '2', '3', '4', '5'],
             ['1', '9007199254740993', '2', '3', '1']]
    for tag, flags in (('', SUMS | POOLED | WEIGHT), ('_round', SUMS | POOLED | WEIGHT | ROUND)):
        out.append(case('weighted_depths%s' % tag, frows, drows, flags=flags, note=dict(weighted_order=[1] if not tag else [])))
    return out


# ---- SITES_ROUND and the consensus letter ---------------------------------------------------------------------------------------------
ROUND_CELLS = ['0.5', '0.5000000000000001', '0.49999999999999994', '1.5', '2.5', '-0.5']
ROUND_TO = [0.0, 1.0, 0.0, 2.0, 2.0, 0.0]


def round_cases():
    out = []
    cells = [(f, '3') for f in ROUND_CELLS] + [('0.5', '0'), ('0.7', '500'), ('0.2', '3')]         # ... depth 0; dropped by the ratio
    for tag, flags in (('round_half_even', SUMS | ROUND), ('round_half_even_pooled', SUMS | ROUND | POOLED), ('letter', SEQ),
                       ('round_weighted', SUMS | ROUND | POOLED | WEIGHT)):
        out.append(one_row(tag, cells, site_ratio=20.0, site_depth=0, flags=flags, note=dict(rounds=True, kept=[True] * 7 + [False, True])))
    # float(round(x)) is +0.0 where rint gives -0.0: eight and more of them go through the pairwise partial sums as they are
    for K in (7, 8, 20):
        for tag, flags in (('', SUMS | ROUND | POOLED), ('_weighted', SUMS | ROUND | POOLED | WEIGHT)):
            out.append(one_row('round_negative_zero_%d%s' % (K, tag), [('-0.3', '2')] * K, flags=flags, note=dict(pooled_bits=[(0, 0.0)])))
    return out


# ---- --max_sites --------------------------------------------------------------------------------------------------------------------
def max_sites_cases():
    """Twelve sites, all kept but row 2 (masked): with group_rows 4 the third kept site is row 3, the last row of the first group,
    and the fourth is row 4, the first row of the second."""
    N, S = 12, 3
    rng = np.random.default_rng(12)
    base_f = [['%.3g' % x for x in rng.random(S)] for _ in range(N)]
    base_d = [[str(int(x)) for x in rng.integers(1, 9, S)] for _ in range(N)]
    mask = np.ones(N, np.uint8)
    mask[2] = 0
    out = []

    def add(name, max_sites, bad=None, raises=None, flags=SUMS | SEQ):
        frows = [list(r) for r in base_f]
        if bad is not None:
            frows[bad][1] = 'x'
        out.append(case(name, frows, base_d, mask=mask, max_sites=max_sites, flags=flags, groups=((4, 0),), note=dict(raises=raises, fill=max_sites)))

    add('max_fill_last_row_of_group', 3)
    add('max_fill_first_row_of_next_group', 4)
    add('max_0', 0)
    add('max_1', 1)
    add('max_12', 12)
    add('max_bad_behind_fill_next_group', 3, bad=4, raises=(1, 4, 1))         # the one row more opens the next group
    add('max_bad_behind_fill_same_group', 4, bad=5, raises=(1, 5, 1))
    add('max_bad_two_behind_fill', 3, bad=5)
    add('max_bad_two_behind_fill_same_group', 4, bad=6)
    add('max_0_bad_row_0', 0, bad=0, raises=(1, 0, 1))
    add('max_0_bad_row_1', 0, bad=1)
    add('max_1_bad_row_1', 1, bad=1, raises=(1, 1, 1))
    add('max_1_bad_row_2', 1, bad=2)
    return out


# ---- where the reference raises: the pool of a site it cannot form ----------------------------------------------------------------------
def refusal_cases():
    N, S = 9, 3
    f0 = [['0.25', '0.5', '0.75'] for _ in range(N)]
    d0 = [['2', '3', '4'] for _ in range(N)]
    out = []

    def add(name, raises, fedit=(), dedit=(), **opts):
        frows, drows = [list(r) for r in f0], [list(r) for r in d0]
        for r, s, c in fedit:
            frows[r][s] = c
        for r, s, c in dedit:
            drows[r][s] = c
        out.append(case(name, frows, drows, groups=((4, 0), (5, 0)), note=dict(raises=raises), **opts))

    W = SUMS | POOLED | WEIGHT
    zero5 = [(5, s, '0') for s in range(S)]
    add('weighted_zero_depth', (6, 5, -1), dedit=zero5, site_depth=0, flags=W)
    add('weighted_zero_depth_masked_site', (6, 5, -1), dedit=zero5, site_depth=0, flags=W, mask=[1, 1, 1, 1, 1, 0, 1, 1, 1])
    add('weighted_depths_cancel', (6, 4, -1), dedit=[(4, 0, '-2'), (4, 1, '2'), (4, 2, '0')], site_depth=-5, flags=W)
    add('weighted_zero_depth_none_kept', None, dedit=zero5, site_depth=1, flags=W)                  # count 0: pooled is 0.0 by rule
    add('weighted_zero_depth_two_rows', (6, 3, -1), dedit=zero5 + [(3, s, '0') for s in range(S)] + [(7, s, '0') for s in range(S)], site_depth=0, flags=W)
    add('unweighted_zero_depth', None, dedit=zero5, site_depth=0, flags=SUMS | POOLED)
    add('weighted_zero_depth_behind_fill', None, dedit=zero5, site_depth=0, flags=W, max_sites=5)
    add('weighted_zero_depth_is_fill_row', (6, 5, -1), dedit=zero5, site_depth=0, flags=W, max_sites=6)
    add('weighted_zero_depth_after_bad_cell', (1, 2, 0), dedit=zero5, fedit=[(2, 0, '0.5x')], site_depth=0, flags=W)
    add('weighted_zero_depth_before_bad_cell', (6, 5, -1), dedit=zero5, fedit=[(6, 0, '0.5x')], site_depth=0, flags=W)
    add('weighted_zero_depth_with_bad_cell', (2, 5, 2), dedit=[(5, 0, '0'), (5, 1, '0'), (5, 2, '0.0')], site_depth=0, flags=W)
    R = SUMS | ROUND
    for cell in ('nan', 'inf', '-inf', '1e400', '-Infinity'):
        add('round_%s' % cell, (3, 3, 1), fedit=[(3, 1, cell)], flags=R)
    add('round_nan_sample_not_kept', (3, 3, 1), fedit=[(3, 1, 'nan')], dedit=[(3, 1, '0')], flags=R)
    add('round_nan_first_of_two_samples', (3, 3, 0), fedit=[(3, 2, 'nan'), (3, 0, 'inf')], flags=R | POOLED)
    add('round_nan_earliest_row', (3, 1, 2), fedit=[(7, 0, 'nan'), (1, 2, 'inf'), (4, 1, 'nan')], flags=R)
    add('round_nan_and_zero_depth_in_one_row', (3, 5, 2), fedit=[(5, 2, 'nan')], dedit=zero5, site_depth=0, flags=R | W)
    add('round_nan_behind_fill', None, fedit=[(3, 1, 'nan')], flags=R, max_sites=3)
    add('round_nan_is_fill_row', (3, 3, 1), fedit=[(3, 1, 'nan')], flags=R, max_sites=4)
    add('round_nan_max_0', None, fedit=[(0, 1, 'nan')], flags=R, max_sites=0)
    add('round_nan_after_bad_cell_same_row', (2, 3, 2), fedit=[(3, 0, 'nan')], dedit=[(3, 2, '')], flags=R)
    # a cell that is no number in each matrix: the reference meets the earlier row, then the earlier sample, then the frequency
    add('bad_cells_depth_row_first', (2, 2, 1), fedit=[(6, 0, 'x')], dedit=[(2, 1, 'x')])
    add('bad_cells_freq_row_first', (1, 2, 1), fedit=[(2, 1, 'x')], dedit=[(6, 0, 'x')])
    add('bad_cells_one_row_depth_sample_first', (2, 4, 0), fedit=[(4, 2, 'x')], dedit=[(4, 0, 'x')])
    add('bad_cells_one_cell_both', (1, 4, 1), fedit=[(4, 1, 'x')], dedit=[(4, 1, 'x')])
    add('no_round_nan', None, fedit=[(3, 1, 'nan')], flags=SUMS | SEQ)
    add('no_round_inf', None, fedit=[(3, 1, 'inf')], flags=SEQ)
    add('no_round_nan_pooled', None, fedit=[(3, 1, 'nan')], flags=SUMS | POOLED, site_maf=0.1)
    return out


# ---- the sums ---------------------------------------------------------------------------------------------------------------------------
def gene_cases():
    """200 sites of 2 samples.  The gene index changes at lane 63 and at lane 0 of the kernel's 64-row steps and in between; a
    gene of one site; a gene that comes back; sites without a gene in front of, between and behind the genes; one gene without a
    site.  With group_rows 45 and 64 genes span group borders."""
    N, S = 200, 2
    rng = np.random.default_rng(200)
    gene = np.full(N, -1, np.int32)
    gene[3:30], gene[30:63], gene[63], gene[64:100], gene[100:120], gene[125:161] = 0, 1, 2, 3, 0, 1
    frows = [['%.3g' % x if r % 3 else '%.17g' % x for x in rng.random(S)] for r in range(N)]
    drows = [[str(int(x)) for x in rng.integers(0, 4, S)] for r in range(N)]
    mask = (rng.random(N) < 0.85).astype(np.uint8)
    mask[[3, 29, 30, 62, 63, 64, 99, 100, 160]] = 1
    for r in (63, 64, 100):
        drows[r] = ['2', '3']
    out = []
    for tag, flags in (('per_gene', SUMS | PER_GENE), ('per_gene_pooled', SUMS | PER_GENE | POOLED), ('genome', SUMS), ('genome_pooled', SUMS | POOLED),
                       ('per_gene_weighted', SUMS | PER_GENE | POOLED | WEIGHT)):
        out.append(case('genes_%s' % tag, frows, drows, mask=mask, site_gene=gene, n_genes=5, flags=flags, groups=((45, 0), (64, 0), (63, 0)),
                        note=dict(genes=True)))
    return out


def snp_maf_cases():
    cells = ['0.01', '0.009999999999999998', '0.010000000000000002', '0.99', '0.9900000000000001', '0.98999999999999999', '0.5', '0', '1']
    expect = [True, False, True, True, False, True, True, False, False]
    out = [case('snp_maf_per_sample', [[c, '0.3'] for c in cells], [['2', '2']] * len(cells), snp_maf=0.01, flags=SUMS, note=dict(snp=expect)),
           case('snp_maf_pooled', [[c] for c in cells], [['2']] * len(cells), snp_maf=0.01, flags=SUMS | POOLED, note=dict(snp=expect)),
           case('snp_maf_zero', [[c] for c in cells], [['2']] * len(cells), snp_maf=0.0, flags=SUMS, note=dict(snp=[True] * 7 + [True, True]))]
    return out


def fused(a, b, c):
    """fma(a, b, c): a * b + c rounded once."""
    if hasattr(math, 'fma'):
        return math.fma(a, b, c)
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def pi_chain(fs, contract):
    """pi += (2 f)(1 - f) over a chain, as written, or with the product fused into the addition (what -ffp-contract=off forbids)."""
    pi = 0.0
    for f in fs:
        pi = fused(2.0 * f, 1.0 - f, pi) if contract else pi + (2.0 * f) * (1.0 - f)
    return pi


def fma_cases():
    """The seed is searched: the chain of sample 0, the chain of the pool and the weighted sum must each come out with other bits
    when the product is fused into the addition."""
    for seed in range(77, 177):
        rng = np.random.default_rng(seed)
        frows = [['%.17g' % x for x in rng.random(2)] for _ in range(40)]
        drows = [[str(int(x)) for x in rng.integers(1, 1000, 2)] for _ in range(40)]
        pooled = [((0.0 + float(a)) + float(b)) / 2 for a, b in frows]
        plain = contracted = 0.0
        for f, d in zip(sum(frows[:20], []), sum(drows[:20], [])):
            plain += int(d) * float(f)
            contracted = fused(float(int(d)), float(f), contracted)
        dsum = sum(int(d) for d in sum(drows[:20], []))
        if all(pi_chain(fs, False) != pi_chain(fs, True) for fs in ([float(a) for a, _ in frows], pooled)) and plain / dsum != contracted / dsum:
            break
    else:
        raise AssertionError('fma_cases')
    return [case('fma_pi_per_sample', frows, drows, flags=SUMS, note=dict(fma='pi')),
            case('fma_pi_pooled', frows, drows, flags=SUMS | POOLED, note=dict(fma='pooled')),
            case('fma_weighted_pool', [sum(frows[:20], [])], [sum(drows[:20], [])], flags=SUMS | POOLED | WEIGHT, note=dict(fma='msum'))]


def depth_sum_cases():
    drows = [['3000000000', '1'], ['3000000000', '4294967295'], ['4611686018427387904', '1'], ['2147483648', '2147483648'], ['5', '4294967296']]
    return [case('depth_sums_past_2p32', [['0.25', '0.5']] * 5, drows, flags=SUMS, note=dict(depth_sum=1 << 32))]


def site_cases(pairwise_sum):
    return (depth_cases() + ratio_cases() + support_cases() + prevalence_cases() + pooled_cases() + pairwise_cases(pairwise_sum) +
            weighted_cases() + round_cases() + max_sites_cases() + refusal_cases() + gene_cases() + snp_maf_cases() + fma_cases() +
            depth_sum_cases())


# ---- strain_tracking.py: the marker calls -------------------------------------------------------------------------------------------
# (frequency cell, depth, x * depth as the interpreter forms it, round() of it)
PRODUCTS = [('0.5', 5, 2.5, 2), ('0.5', 7, 3.5, 4), ('0.07', 100, 7.000000000000001, 7), ('0.29', 100, 28.999999999999996, 29),
            ('0.15', 30, 4.5, 4), ('0.35', 10, 3.5, 4)]
Marker = collections.namedtuple('Marker', 'name frows drows minor major min_freq min_reads allele_prev note')


def marker_cases():
    """Sample 0 carries the chosen cell; sample 1 has the major allele alone and sample 2 the minor allele alone, so that every
    site has two letters and is reported with its counts whatever sample 0 is called."""
    out = []

    def table(name, cells, min_freq, min_reads, allele_prev=3, note=None, minor=0, major=1):
        frows = [[f, '0', '1'] for f, _ in cells]
        drows = [[str(d), '1000', '1000'] for _, d in cells]
        n = len(cells)
        out.append(Marker(name, frows, drows, np.full(n, minor, np.uint8), np.full(n, major, np.uint8), min_freq, min_reads, allele_prev, note or {}))

    # x on min_freq and either side of it, for the minor allele (x = f) and for the major (x = 1 - f)
    fr = [('0.1', 100), ('0.09999999999999999', 100), ('0.10000000000000002', 100), ('0.9', 100), ('0.89999999999999991', 100), ('0.90000000000000013', 100)]
    table('min_freq', fr, 0.1, 1, note=dict(has_minor=[True, False, True, True, True, True], has_major=[True, True, True, False, True, False]))
    # round(x * d) against min_reads on the value and its neighbours
    for f, d, prod, r in PRODUCTS:
        for mr in (r - 1, r, r + 1):
            table('reads_%s_x_%d_min_%d' % (f, d, mr), [(f, d)], 0.01, mr, note=dict(product=(f, d, prod, r), has_minor=[r >= mr]))
    table('depth_zero', [('0.5', 0), ('0.5', 4)], 0.1, 1, note=dict(total=[2, 3]))
    table('both_alleles', [('0.5', 10), ('0.3', 10), ('0', 10), ('1', 10)], 0.1, 2, note=dict(has_minor=[True, True, False, True], has_major=[True, True, True, False]))
    # carriers of the rarer allele: allele_prev of them, one fewer, one more
    S = 9
    frows, drows = [], []
    for k in (1, 2, 3, 4):
        frows.append(['1' if s % 2 == 0 and s // 2 < k else '0' for s in range(S)])
        drows.append(['10'] * S)
    for prev in (1, 2, 3):
        out.append(Marker('carriers_prev_%d' % prev, frows, drows, np.full(4, 2, np.uint8), np.full(4, 3, np.uint8), 0.1, 3, prev,
                          dict(markers=[k <= prev for k in (1, 2, 3, 4)])))
    # every fold of the two alleles onto A, T, C, G
    folds = [(a, b) for a in range(4) for b in range(4)]
    cells = [('0.4', 10)] * len(folds)
    frows = [[f, '0', '1'] for f, _ in cells]
    drows = [[str(d), '10', '10'] for _, d in cells]
    out.append(Marker('folds', frows, drows, np.array([a for a, _ in folds], np.uint8), np.array([b for _, b in folds], np.uint8), 0.1, 3, 3,
                      dict(markers=[a != b for a, b in folds])))
    return out


# ---- the device's own converters at the borders of their fast paths ------------------------------------------------------------------
def float_cells():
    """-> [(cell, whether the device converts it itself)]; every cell is a float() literal."""
    out = []
    lim = 1 << 53
    for v in (lim - 1, lim, lim + 1):
        s = str(v)
        fast = v < lim
        out += [(s, fast), ('000' + s, fast), ('0.' + s, fast), ('-' + s, fast), (s + 'e-22', fast), (s + 'e22', fast), (s + 'e23', False)]
        out += [(s[:k] + '.' + s[k:], fast) for k in range(1, len(s))]
    out += [('0.50000000000000000000', False), ('0.5000000000000000', True), ('0.500000000000000000', False), ('00000000000000000000.5', True),
            ('1.5e23', True), ('1e23', False), ('1e22', True), ('15e22', True), ('1.5e-22', False), ('15e-23', False), ('1e-22', True), ('1e-23', False),
            ('12345e-27', False), ('12345e-22', True), ('12345e-23', False), ('1.2345e-18', True), ('1.2345e-19', False), ('1.2345e26', True),
            ('1.2345e27', False), ('1e022', True), ('1e0022', False), ('1e-022', True), ('1E+022', True), ('1e+0022', False), ('0e999', True),
            ('0.0e-999', True), ('-0e5', True), ('0e9999', False), ('0.000e+999', True), ('5.', False), ('.5', False), ('-.5', False), ('5.e3', False)]
    rng = np.random.default_rng(53)
    for m in rng.integers(10 ** 14, lim, 40).tolist():       # one IEEE division / multiplication with a rounded result
        out += [('%de-22' % m, True), ('%de-%d' % (m, 1 + m % 21), True), ('%de22' % m, True)]
    return out


REFUSED_FLOATS = ['1e', '1e+', '+', '-', '1.2.3', '--1', 'e5', '.', '1e5.0']


def int_cells():
    return [('999999999999999999', True), ('100000000000000000', True), ('-999999999999999999', True), ('+999999999999999999', True),
            ('1000000000000000000', False), ('9223372036854775807', False), ('-9223372036854775808', False), ('-0', True), ('+0', True),
            ('000000000000000000', True), ('0000000000000000001', False), ('-1000000000000000000', False), ('12345678901234567', True)]


REFUSED_INTS = ['5.', '1e3', '+', '-', '--1', '1.0', '']


# ---- the commands ---------------------------------------------------------------------------------------------------------------------
ROUND_EXIT = "\nError: %s/snps_freq.txt, line %d: sample %s: the frequency is not a finite number, so --consensus cannot round it\n"
ZERO_DEPTH_EXIT = "\nError: %s/snps_depth.txt, line %d: the depths of the samples kept at the site sum to 0, so --weight_by_depth has no frequency for it\n"


def with_cell(species, which, line, field, cell):
    """A species of the golden vectors (its files as strings) with one cell of snps_<which>.txt replaced: line 0 is the header,
    field 0 the site id."""
    sp = dict(species)
    rows = sp[which].split('\n')
    f = rows[line].split('\t')
    f[field] = cell
    rows[line] = '\t'.join(f)
    sp[which] = '\n'.join(rows)
    return sp
