"""A vectorised model of the merge site arithmetic (merge_sites.hip) and tables chosen to sit ON its decisions and one step to
either side, where seeded Poisson tables almost never land.  Plain numpy and the constructions that find the rows -- nothing here
knows the kernels.  tests/test_merge_cases_host.py ties the model to oracle/merge_oracle.py site by site and asserts with the
model alone that every case says what its claims say; tests/test_gpu_merge_borders.py lays the same groups over every kernel
form, several grid passes and several chunks deep, and holds the device to the model at every site.

A Group is (name, args, mean, counts, claims, marks): the merge arguments, the samples' mean depths, counts[S, k, 4], claims =
[(field, rows, expected)] -- what the model must return at those rows, written down from the case's construction and not from
the model -- and marks = {kind: rows} for the coverage the host check asks of every form.  Every builder takes the sample count
S, so the same decisions fall to every form."""
import collections
import itertools

import numpy as np

Group = collections.namedtuple('Group', 'name args mean counts claims marks')
DEFAULTS = dict(snp_type=['any'], allele_freq=0.01, site_depth=1, site_ratio=2.0, site_prev=0.0)
SNP_NAMES = [None, 'mono', 'bi', 'tri', 'quad']
NONE = 255
BIG = 1 << 28                      # at and above this a count takes the 64-bit route in every form (2^28 / 2^16 / 2^8)
TOP = (1 << 31) - 1                # the table readers bound counts to 31 bits
DEEP = float(np.nextafter(64.0, 65.0))          # the smallest mean depth that rules the byte-packed form out
LIMIT_MEANS = [2.5, 3.7, 0.1, 7.0 / 3.0, 1e-300, 1e300, 12.0, 1.0, 4.999999999999999, 5.000000000000001]     # test_depth_ratio_limits
FREQ_LITERALS = [(0.01, 1, 100), (0.05, 1, 20), (0.2, 1, 5), (0.3333333333333333, 1, 3), (0.5, 1, 2), (1.0, 1, 1)]
PERMS = list(itertools.permutations(range(4)))

# the forms and the sample counts they are tested at: (S, deep) -- deep: one mean of DEEP, which takes 65..128 samples to the split form
FORM_TABLE = [(1, False), (8, False), (9, False), (64, False), (65, False), (72, False), (73, False), (128, False),
              (65, True), (111, True), (112, True), (129, False), (200, False)]
# sample counts at which k / S is exactly a site_prev that is no power of two (3/5 = 0.6, 19/20 = 0.95): the rows that tell the
# reference's pass / float(S) from any other way to form the prevalence -- one count or more for every form
PREV_TABLE = [(5, False), (20, False), (40, False), (60, False), (100, False), (100, True), (120, True), (140, False)]


# ---- the model --------------------------------------------------------------------------------------------------------------------
def model(counts, mean, args):
    """GenomicSite over whole tables: counts[S, n, 4], mean[S] -> every array Context.merge_sites returns, and 'raises': the first
    site at which compute_prevalence divides by a mean depth of zero (-1: none; the arrays say nothing from there on).  The
    operations are the reference's (midas/merge/snps.py, line numbers as in oracle/merge_oracle.py)."""
    c = np.asarray(counts).astype(np.uint64)
    S, n, _ = c.shape
    mean = np.asarray(mean, np.float64)
    pooled = c.sum(axis=0, dtype=np.uint64)                                  # compute_pooled_counts :38-43
    depth = pooled.sum(axis=1, dtype=np.uint64)
    has = depth > 0
    freqs = pooled.astype(np.float64) / np.where(has, depth, 1).astype(np.float64)[:, None]       # call_alleles :49-76
    order = np.argsort(-freqs, axis=1, kind='stable')                        # sorted(..., reverse=True) is stable: ties keep A,C,G,T
    f = np.take_along_axis(freqs, order, axis=1)
    major = np.where(has & (f[:, 0] > 0), order[:, 0], NONE).astype(np.uint8)
    minor = np.where(has & (f[:, 1] > 0), order[:, 1], NONE).astype(np.uint8)
    snp = np.zeros(n, np.uint8)
    for rank in range(4):                                                    # from the rarest up: the rarest that reaches it names the type
        snp[has & (f[:, rank] >= args['allele_freq'])] = rank + 1

    def of(allele):                                                          # c[s, i, allele[i]], and 0 where the allele is None
        j = np.broadcast_to(np.minimum(allele, 3).astype(np.int64)[None, :, None], (S, n, 1))
        return np.where((allele == NONE)[None, :], np.uint64(0), np.take_along_axis(c, j, axis=2)[:, :, 0])

    minor_count = of(minor)                                                  # compute_per_sample_mafs :78-91 (no major: no minor either)
    d = of(major) + minor_count
    di = d.astype(np.int64)
    deep_enough = di >= int(args['site_depth'])                              # compute_prevalence :93-104
    with np.errstate(divide='ignore', invalid='ignore'):
        over = d.astype(np.float64) / mean[:, None] > args['site_ratio']
    zero = (mean == 0.0)[:, None] & deep_enough
    ok = (deep_enough & ~over & ~(mean == 0.0)[:, None]).sum(axis=0)
    flag = np.zeros(n, np.uint8)                                             # flag :106-114
    low = ok / float(S) < args['site_prev']
    wanted = np.array(['any' in args['snp_type'] or SNP_NAMES[t] in args['snp_type'] for t in range(5)])
    flag[~low & ~wanted[snp]] = 2
    flag[low] = 1
    hit = np.flatnonzero(zero.any(axis=0))
    return dict(major=major, minor=minor, snp_type=snp, flag=flag, count_samples=ok.astype(np.uint32), pooled=pooled,
                depth=d.astype(np.uint32), minor_count=minor_count.astype(np.uint32), raises=int(hit[0]) if hit.size else -1)


FIELDS = ('major', 'minor', 'snp_type', 'flag', 'count_samples', 'pooled', 'depth', 'minor_count')


def form_of(S, means):
    """launch_merge_kernel's choice, as its trace line names it."""
    if S <= 64:
        return 'regs32' if S <= 8 else 'regs16'
    if S <= 128 and all(m <= 64.0 for m in means):
        return 'bytes S=%d' % ((S + 7) // 8 * 8)
    return 'split G=%d' % (8 if S < 112 else 16)


def sites_per_block(form):
    return 64 if form.startswith('split') else 256


def keeps(d, mean, ratio, depth):
    """compute_prevalence's two tests on Python numbers."""
    return d >= depth and not (d / mean > ratio)


def limits(mean, ratio, depth, top=2 * TOP):
    """-> (lo, hi): the depths a sample of a positive mean depth keeps, by bisection with the reference's expression."""
    assert mean > 0 and not (0 / mean > ratio)
    if not (top / mean > ratio):
        return max(depth, 0), top
    a, b = 0, top
    while b - a > 1:
        m = (a + b) // 2
        if m / mean > ratio:
            b = m
        else:
            a = m
    return max(depth, 0), a


# ---- pooled counts laid over S samples -----------------------------------------------------------------------------------------------
def spread(pooled, S, way):
    """pooled[k, 4] -> counts[S, k, 4] with those sums.  way 0: a site's counts all in one sample; 1: as even as it goes over all
    samples (no single count decides); 2: the site scaled by a whole factor (count / depth is the same real number, so the same
    double) until its largest count is at least BIG, that count alone in one sample and the others in the next."""
    pooled = np.asarray(pooled, np.int64).reshape(-1, 4)
    k = pooled.shape[0]
    c = np.zeros((S, k, 4), np.int64)
    for i, p in enumerate(pooled):
        if way == 0:
            c[(3 * i + 1) % S, i] = p
        elif way == 1:
            c[:, i] = p // S
            for a in range(4):
                c[(np.arange(int(p[a] % S)) + i + a) % S, i, a] += 1
        elif p.max() > 0:
            big = p * -(-BIG // int(p.max()))
            a = int(np.argmax(p))
            c[i % S, i, a] += big[a]
            big[a] = 0
            c[(i + 1) % S, i] += big
    assert c.max(initial=0) <= TOP and (c.sum(axis=0) % np.maximum(pooled, 1) == 0).all()
    return c


def pooled_group(name, S, pooled, call_claims=(), flag_claims=(), marks=None, mean=None, fixed=None, fixed_claims=(), **args):
    """The pooled rows three ways (rows w * k + i), then the rows given sample by sample (fixed[S, j, 4]).  call_claims speak of
    what follows from the pooled counts alone and hold for every way; flag_claims of prevalence too: ways 0 and 1."""
    pooled = np.asarray(pooled, np.int64).reshape(-1, 4)
    k = pooled.shape[0]
    counts = np.concatenate([spread(pooled, S, w) for w in range(3)] + ([fixed] if fixed is not None else []), axis=1)
    claims = [(f, [w * k + r for r in rows], exp) for w in range(3) for f, rows, exp in call_claims]
    claims += [(f, [w * k + r for r in rows], exp) for w in range(2) for f, rows, exp in flag_claims]
    claims += [(f, [3 * k + r for r in rows], exp) for f, rows, exp in fixed_claims]
    m = {kind: [w * k + r for w in range(3) for r in rows] for kind, rows in (marks or {}).items()}
    m['fallback'] = [2 * k + i for i in range(k) if pooled[i].max() > 0]
    return Group(name, dict(DEFAULTS, **args), [10.0] * S if mean is None else list(mean), counts, claims, m)


# ---- order ------------------------------------------------------------------------------------------------------------------------
TIE_SETS = {'two_equal': [(5, 5, 3, 1), (5, 3, 3, 1), (5, 3, 1, 1)], 'two_pairs': [(5, 5, 2, 2)], 'three_equal': [(5, 5, 5, 1), (5, 1, 1, 1)],
            'four_equal': [(5, 5, 5, 5)], 'at_zero': [(5, 3, 0, 0), (5, 5, 0, 0), (5, 0, 0, 0), (5, 5, 5, 0)], 'depth_zero': [(0, 0, 0, 0)]}


def order_group(S):
    """All 24 orders of four distinct counts, every tie pattern in every position, depth 0, one allele only.  Expected: sort by
    (-count, A<C<G<T); an allele of count 0 is never called."""
    rows, marks = [tuple(10 * (4 - p[a]) for a in range(4)) for p in PERMS], {}
    for kind, sets in TIE_SETS.items():
        arr = sorted(set(q for v in sets for q in itertools.permutations(v)))
        marks['tie_' + kind] = list(range(len(rows), len(rows) + len(arr)))
        rows += arr
    major, minor = [], []
    for p in rows:
        o = sorted(range(4), key=lambda a: (-p[a], a))
        major.append(o[0] if p[o[0]] > 0 else NONE)
        minor.append(o[1] if p[o[1]] > 0 else NONE)
    every = list(range(len(rows)))
    return pooled_group('order', S, rows, [('major', every, major), ('minor', every, minor)], marks=marks)


# ---- allele_freq ------------------------------------------------------------------------------------------------------------------
def _even(total, n):
    return [total // n + (1 if j < total % n else 0) for j in range(n)] if n else []


def freq_rows(rank, a, b):
    """-> [below, on, above] (above may be missing): pooled counts by rank of one depth, where the count at `rank` is one below
    a/b of the depth, exactly a/b of it, one above; every rarer allele stays below a/b in all of them."""
    for want_above in (True, False):
        for m in range(1, 40):
            c, D = a * m, b * m
            rest = D - c
            if rank == 0:
                # the major allele holds c, the other three share the rest as evenly as it goes.  The step is traded with
                # rank 1: below, rank 1 takes the count the major allele gives up and must still stay under it (v[0] + 1 <=
                # c - 1); above, rank 1 gives one up (v[0] >= 1)
                v = _even(rest, 3)
                if v[0] + 1 > c - 1 or (want_above and (v[0] < 1 or c + 1 > D)):
                    continue
                on = [c] + v
                partner = 1
            else:
                # the commoner ranks hold at least c + 1 (so that c + 1 at `rank` keeps its rank; without an above row c is
                # enough), the rarer ones at most c - 1, as many as the depth leaves (`spare`); what is over goes to the major
                # allele.  The step is traded with the major allele: it takes the count below and gives it above, hence c + 2
                common = [c + 2] + [c + 1] * (rank - 1) if want_above else [c] * rank
                spare = rest - sum(common)
                if spare < 0:
                    continue
                rare = min((3 - rank) * (c - 1), spare)
                common[0] += spare - rare
                on = common + [c] + _even(rare, 3 - rank)
                partner = 0
            out = []
            for step in (-1, 0, 1) if want_above else (-1, 0):
                v = list(on)
                v[rank] += step
                v[partner] -= step
                out.append(tuple(v))
            assert all(sum(v) == D and min(v) >= 0 and max(v) < 256 for v in out), out
            return out
    return None


def freq_groups(S):
    out = []
    for lit, a, b in FREQ_LITERALS:
        rows, claims, exact = [], [], []
        for rank in range(4):
            tri = freq_rows(rank, a, b)
            if tri is None:
                continue
            assert tri[1][rank] / sum(tri[1]) == lit and float(tri[1][rank]) / sum(tri[1]) >= lit
            perm = PERMS[(7 * rank + 5 * b) % 24]                           # which allele holds which rank: not always A > C > G > T
            at = len(rows)
            rows += [tuple(v[perm[al]] for al in range(4)) for v in tri]
            claims.append(('snp_type', list(range(at, at + len(tri))), [rank, rank + 1, rank + 1][:len(tri)]))
            exact.append(at + 1)
        out.append(pooled_group('allele_freq_%g' % lit, S, rows, claims, marks=dict(exact_freq=exact), allele_freq=lit))
    zero = [(7, 0, 0, 0), (0, 0, 0, 9), (1, 1, 1, 1), (0, 0, 0, 0)]
    out.append(pooled_group('allele_freq_0', S, zero, [('snp_type', [0, 1, 2, 3], [4, 4, 4, 0])], allele_freq=0.0))
    above = [(5, 0, 0, 0), (2, 2, 2, 2), (0, 3, 1, 0)]
    out.append(pooled_group('allele_freq_above_1', S, above, [('snp_type', [0, 1, 2], [0, 0, 0])], allele_freq=float(np.nextafter(1.0, 2.0))))
    return out


# ---- the type mask ----------------------------------------------------------------------------------------------------------------
MASKS = [['mono'], ['bi'], ['tri'], ['quad'], ['bi', 'tri'], ['mono', 'bi', 'tri', 'quad'], ['any']]
TYPE_ROWS = [(0, 0, 0, 0), (0, 10, 0, 0), (5, 0, 0, 5), (3, 0, 4, 3), (2, 3, 2, 3)]      # None .. quad at allele_freq 0.2 (2/10 is on it)


def mask_groups(S):
    """site_depth 0, so that the site of depth 0 passes in every sample: type None, kept by 'any' and flagged 2 by every other
    mask.  The last row holds 30 x A in every sample: mono, three times every mean, so no sample passes and the flag is 1
    whether its type is wanted or not."""
    out = []
    fixed = np.zeros((S, 1, 4), np.int64)
    fixed[:, 0, 0] = 30
    for mask in MASKS:
        flags = [0 if 'any' in mask or SNP_NAMES[t] in mask else 2 for t in range(5)]
        out.append(pooled_group('mask_' + '+'.join(mask), S, TYPE_ROWS, [('snp_type', list(range(5)), list(range(5)))],
                                [('flag', list(range(5)), flags)], fixed=fixed, fixed_claims=[('flag', [0], [1]), ('snp_type', [0], [1])],
                                snp_type=mask, allele_freq=0.2, site_depth=0, site_prev=0.5))
    return out


# ---- prevalence -------------------------------------------------------------------------------------------------------------------
def prev_settings(S):
    """-> [(site_prev, k, flags of k - 1, k, k + 1 passing samples, exact)]"""
    out = []
    for p in (0.95, 0.5, 0.6, 1.0):
        k = int(round(p * S))
        if k >= 1 and k / float(S) == p and (p != 0.6 or S == 5) and (p != 0.95 or S % 20 == 0):
            out.append((p, k, [1, 0, 0], True))
    k = max(1, S // 2)
    out.append((float(np.nextafter(k / float(S), 0.0)), k, [1, 0, 0], False))
    out.append((float(np.nextafter(k / float(S), 2.0)), k, [1, 1, 0], False))      # (towards 2: k / S is 1.0 with one sample)
    return out


def prev_groups(S):
    """j passing samples hold 5 x A (2^28 x A in the third block of rows) and the others nothing: the first j samples, the last j,
    then the first j again with the large count."""
    out = []
    for p, k, flags, exact in prev_settings(S):
        js = [j for j in (k - 1, k, k + 1) if 0 <= j <= S]
        fixed = np.zeros((S, 3 * len(js), 4), np.int64)
        claims = []
        for w in range(3):
            for n, j in enumerate(js):
                who = np.arange(S - j, S) if w == 1 else np.arange(j)
                fixed[who, w * len(js) + n, 0] = BIG if w == 2 else 5
            rows = [w * len(js) + n for n in range(len(js))]
            claims += [('flag', rows, flags[:len(js)]), ('count_samples', rows, js)]
        on = [w * len(js) + js.index(k) for w in range(3)]
        g = pooled_group('prev_%r' % p, S, np.zeros((0, 4)), fixed=fixed, fixed_claims=claims, site_prev=p, site_ratio=1e18)
        g.marks.update(exact_prev=on if exact else [], fallback=[2 * len(js) + n for n in range(len(js)) if js[n] > 0])
        out.append(g)
    return out


# ---- per-sample limits ------------------------------------------------------------------------------------------------------------
def limits_group(S, deep=False):
    """Every sample at lo - 1, lo, hi, hi + 1 of its own interval (A only, so depth = its count), four rows that start the cycle
    at another place for each sample; expected count_samples from the reference's expression on Python numbers."""
    args = dict(DEFAULTS, site_depth=1, site_ratio=2.0)
    mean = [LIMIT_MEANS[s % len(LIMIT_MEANS)] for s in range(S)]
    if 64 < S <= 128 and not deep:         # the byte form is wanted: no mean above 64
        mean = [64.0 if m == 1e300 else m for m in mean]
    if deep:
        mean[14] = DEEP
    fixed = np.zeros((S, 4, 4), np.int64)
    for s in range(S):
        lo, hi = limits(mean[s], args['site_ratio'], args['site_depth'])
        for row in range(4):
            fixed[s, row, 0] = min(max([lo - 1, lo, hi, hi + 1][(row + s) % 4], 0), TOP)
    expected = [sum(keeps(int(fixed[s, row, 0]), mean[s], args['site_ratio'], args['site_depth']) for s in range(S)) for row in range(4)]
    return Group('limits', args, mean, fixed, [('count_samples', [0, 1, 2, 3], expected)], {})


def groups(S, deep=False):
    """Every group for S samples.  deep: one sample's mean is DEEP (65..128 samples then take the split form)."""
    out = [order_group(S)] + freq_groups(S) + mask_groups(S) + prev_groups(S)
    if deep:
        for g in out:
            g.mean[S // 3] = DEEP
    return out + [limits_group(S, deep)]


# ---- tables for the device ----------------------------------------------------------------------------------------------------------
def random_sites(seed, S, n):
    """Shallow seeded sites: every count fits a byte."""
    rng = np.random.default_rng(seed)
    return (rng.poisson(6.0, (S, n, 4)) * (rng.random((S, n, 4)) < 0.5)).astype(np.int64)


def lay(chosen, fill, pass_sites):
    """fill[S, n, 4] with runs of the chosen sites written over it: at the start, centred on every multiple of pass_sites, and
    at the end where the last of those leaves room.  No run is wider than a pass, so none overwrites another; each takes up the
    chosen sites (cyclically) where the one before stopped -- 97 further on when a run holds them all, so that another site
    meets the border each time.  Every chosen site is in the table at least once; the fill's seeded sites lie between."""
    S, k = chosen.shape[:2]
    n = fill.shape[1]
    t = fill.copy()
    w, w0 = min(k, pass_sites), min(k, pass_sites // 2)
    runs = [(0, w0)] + [(p - w // 2, min(p - w // 2 + w, n)) for p in range(pass_sites, n, pass_sites)]
    if n - w0 >= runs[-1][1]:
        runs.append((n - w0, n))
    cursor, seen = 0, np.zeros(k, bool)
    for lo, hi in runs:
        idx = (cursor + np.arange(hi - lo)) % k
        t[:, lo:hi] = chosen[:, idx]
        seen[idx] = True
        cursor += (hi - lo) + (97 if hi - lo >= k else 0)
    assert seen.all() and all(a[1] <= b[0] for a, b in zip(runs, runs[1:]))
    return t.astype(np.uint32)


def zero_positions(S, form):
    """Where the sample of mean 0 goes: first, middle, last -- and in the split form wave s % G: wave 0, a middle wave, the last."""
    z = [0, S // 2, S - 1]
    if form.startswith('split'):
        G = int(form.split('=')[1])
        z += [G // 2, G - 1]
    return sorted(set(z))


def zero_mean_tables(S, z, zero, n, plant, deep=False, seed=5):
    """-> [(name, counts, mean, args, first raising site)].  Sample z has mean `zero` and no counts but where planted: every sample
    holds 3 x A there and z holds 2 (site_depth is 2) -- in the rotated table the earliest planted site holds 2^28 x A in z (the
    64-bit route).  Site 5 holds 1 x A in z, below site_depth: it does not raise.  Table j keeps plant[j:], so each of them is
    the earliest once.  deep: the next sample's mean is DEEP.  Last: site_depth 0, nothing planted: sample z reaches the division at site 0 with depth 0."""
    base = random_sites(seed, S, n)
    base[z] = 0
    base[:, 5] = 0
    base[:, 5, 0] = 1
    mean = [10.0] * S
    if deep:
        mean[(z + 1) % S] = DEEP
    mean[z] = zero
    args = dict(DEFAULTS, site_depth=2)
    out = []
    for j in range(len(plant)):
        for big in (False, True):
            c = base.copy()
            for q in plant[j:]:
                c[:, q] = 0
                c[:, q, 0] = 3
                c[z, q, 0] = 2
            if big:
                c[z, plant[j], 0] = BIG
            out.append(('zero_s%d_from%d%s' % (z, plant[j], '_big' if big else ''), c.astype(np.uint32), mean, args, plant[j]))
    out.append(('zero_s%d_depth0' % z, base.astype(np.uint32), mean, dict(DEFAULTS, site_depth=0), 0))
    return out
