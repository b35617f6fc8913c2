"""Chosen profiles for merge_species.py on the device (midas_amd/csrc/species_merge.hip): every case puts rows, values, ids or
bytes ON a border of one of its kernels or of the host writer, where the random profiles of tests/test_gpu_merge_species.py never
land.  Data and builders only -- nothing here touches a device.  The expectation of a case is never written down here: it is
what tests/merge_species_model.py (M.merge / M.first_error) makes of the case's profiles.  tests/test_merge_species_cases_host.py
asserts that every case sits on what it says it sits on; tests/test_gpu_merge_species_borders.py holds the device to the model.

A case is a dict:
  name, family   'rows/513': the family is the name's prefix
  ids            the species ids of species_info.txt, in row order
  sample_ids, profiles   one text a sample
  sample_depth
  forms          the runs of the case: a list of (keyword arguments of Context.species_merge, lds_rows or None); every run must
                 equal the model (and so every other run)
  refused        None, or True: M.first_error names (reason, sample, line)
  on             what the case is meant to sit on, in words
and whatever its family's assertions need (chain shapes, designed values, the writer's threads).

The families:
  rows/    a. R = 3 at S = 511 ... 4096: the bitonic sort in LDS up to n_pow2 = 4096, sm_pairwise_sum's stack five frames deep
  switch/  b. the LDS form and the long-row form (three radix passes, sm_long_median_kernel) at the default bound, at S and S - 1,
              and with 1 ... 5 species (row_bits 1, 1, 2, 2, 3)
  rowsof/  c. designed rows at S = 1 ... 17: -0.0, negatives, ties, overflow, doubles that differ in one 32-bit half, subnormals
  round/   d. sm_round2 on halves, S = 1
  prev/    e. prevalence 0 and S, coverages on the depth and one ulp under it, five depths; the stable order
  table/   f. the lookup table: one full chain, a chain that wraps, the growth borders, ids that are refused
  fields/  g. the sixteen residues of the fields kernel's 16-byte words, wide headers, empty cells, line ends, header look-alikes
  write/   h. the writer's row blocks in two waves and in one
"""
import math

import numpy as np

from tests import merge_species_model as M

MASK64 = (1 << 64) - 1
HEAD = '\t'.join(M.COLUMNS) + '\n'


# ---- the mirror of midas_amd/csrc/species_table.h (held to the C++ by tests/test_species_table_host.py) ---------------------------
def raw(s):
    return s.encode() if isinstance(s, str) else bytes(s)


def sm_hash(name):
    """FNV-1a 64 over the bytes, then MurmurHash3's three-step finaliser."""
    h = 0xCBF29CE484222325
    for c in raw(name):
        h = ((h ^ c) * 0x100000001B3) & MASK64
    h ^= h >> 33
    h = (h * 0xFF51AFD7ED558CCD) & MASK64
    h ^= h >> 33
    h = (h * 0xC4CEB9FE1A85EC53) & MASK64
    h ^= h >> 33
    return h


def table_size(n_ids):
    size = 16
    while size < 2 * n_ids + 2:
        size *= 2
    return size


def home(name, size):
    return (sm_hash(name) & 0xFFFFFFFF) & (size - 1)


def table_of(ids):
    """-> (size, slot[size] = species + 1 or 0, at[species] = its slot); ValueError for an id listed twice."""
    size = table_size(len(ids))
    slot, at = [0] * size, []
    for g, name in enumerate(ids):
        k = home(name, size)
        while slot[k]:
            if raw(ids[slot[k] - 1]) == raw(name):
                raise ValueError("twice")
            k = (k + 1) & (size - 1)
        slot[k] = g + 1
        at.append(k)
    return size, slot, at


def probe(ids, name):
    """The slots sm_lookup_kernel reads for `name`, in order -> (slots, the species found or None)."""
    size, slot, _ = table_of(ids)
    k, seen = home(name, size), []
    while True:
        seen.append(k)
        if slot[k] == 0:
            return seen, None
        if raw(ids[slot[k] - 1]) == raw(name):
            return seen, slot[k] - 1
        k = (k + 1) & (size - 1)


# ---- builders --------------------------------------------------------------------------------------------------------------------
def profiles_from(ids, cov_texts, ab_texts, reads_texts, order=None, header=None, extra_columns=None, eol='\n', final_eol=True):
    """The samples' profile texts from [species][sample] matrices of spellings.  order[s]: the species of sample s's rows, in file
    order (default: the ids' order); header: the header's cells (default the four named ones), a named column takes the row's
    value wherever it stands, any other cell extra_columns(name, field, species, sample) (default 'x')."""
    header = list(M.COLUMNS) if header is None else list(header)
    out = []
    for s in range(len(cov_texts[0]) if ids else 0):
        lines = ['\t'.join(header)]
        for g in (order[s] if order is not None else range(len(ids))):
            named = dict(species_id=ids[g], count_reads=reads_texts[g][s], coverage=cov_texts[g][s], relative_abundance=ab_texts[g][s])
            lines.append('\t'.join(named[c] if c in named else (extra_columns(c, f, g, s) if extra_columns else 'x') for f, c in enumerate(header)))
        out.append(eol.join(lines) + (eol if final_eol else ''))
    return out


def sample_names(n):
    return ['s%04d' % k for k in range(n)]


def lds_form(n_samples, lds_bound=0):
    """What midas_species_merge decides: rows of up to min(bound or 4096, 4096) samples are sorted in LDS."""
    return n_samples <= min(lds_bound or 4096, 4096)


def case(name, ids, profiles, on, sample_depth=1.0, forms=None, refused=None, **more):
    S = len(profiles)
    forms = [({}, lds_form(S))] if forms is None else forms
    out = dict(name=name, family=name.split('/')[0], ids=list(ids), sample_ids=sample_names(S), profiles=list(profiles), sample_depth=sample_depth,
               forms=forms, refused=refused, on=on)
    out.update(more)
    return out


def both_forms(S, chunks=(0,)):
    """The LDS form and, from two samples on, the long-row form of the same rows."""
    forms = [(dict(chunk_bytes=c), True) for c in chunks]
    if S > 1:
        forms += [(dict(lds_bound=1, chunk_bytes=c), False) for c in chunks]
    return forms


# ---- a, b: long rows of mixed values ---------------------------------------------------------------------------------------------------
def leaf_sum(a):
    """numpy's pairwise_sum below its block size: eight lanes, then the tail."""
    n = len(a)
    if n < 8:
        res = 0.0
        for x in a:
            res += x
        return res
    r = list(a[:8])
    i = 8
    while i < n - n % 8:
        for j in range(8):
            r[j] += a[i + j]
        i += 8
    res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    for x in a[i:]:
        res += x
    return res


def halving_sum(a, cut8):
    """numpy's add.reduce by halves down to 128 values; cut8: the left half is cut at a multiple of eight, as numpy does."""
    n = len(a)
    if n <= 128:
        return leaf_sum(a)
    n2 = n // 2
    if cut8:
        n2 -= n2 % 8
    return halving_sum(a[:n2], cut8) + halving_sum(a[n2:], cut8)


def sum_orders(values):
    """-> (np.add.reduce, left to right, halves that are not cut at multiples of eight, one eight-lane leaf over the whole row)."""
    a = [float(v) for v in values]
    left = 0.0
    for x in a:
        left += x
    return float(np.add.reduce(np.array(a, np.float64))), left, halving_sum(a, False), leaf_sum(a)


def cut_matters(n):
    """Whether numpy's cut of a left half at a multiple of eight moves any border of a reduce over n values.  It moves none at
    2^k and 2^k + 1 values (every left half is a multiple of eight by itself): there, halves that are not cut ARE numpy's sum."""
    if n <= 128:
        return False
    n2 = n // 2
    return n2 % 8 != 0 or cut_matters(n2) or cut_matters(n - n2)


def order_sensitive(values):
    """numpy's sum of the row differs in bits from the left-to-right sum, from one leaf over the whole row and -- where the cut at
    multiples of eight moves a border at all -- from the halves that are not cut."""
    got = [np.float64(x).view(np.uint64) for x in sum_orders(values)]
    return got[0] != got[1] and got[0] != got[3] and (got[0] != got[2]) == cut_matters(len(values))


def mixed_values(rng, n):
    """M.palette, a quarter of it negative, a quarter replaced by 17-digit values (the host's parser)."""
    out = M.palette(rng, n)
    for k in range(n):
        pick = int(rng.integers(0, 4))
        if pick == 0:
            out[k] = '-' + out[k]
        elif pick == 1:
            out[k] = '%.17g' % (float(rng.random()) * 10.0 ** int(rng.integers(-3, 4)) * (-1.0 if rng.random() < 0.25 else 1.0))
    return out


# seeds at which some coverage row and some abundance row is order_sensitive (asserted by the host test).  Of the sizes at the
# borders of n_pow2 only 511 has a cut to move; 1000 and 4090 are here for the cut alone (500 -> 496; 2045 -> 2040, 1022 -> 1016 ...)
ROW_SEEDS = {511: 2, 512: 1, 513: 1, 1000: 1, 1024: 1, 1025: 2, 2049: 1, 4090: 1, 4096: 1, 4097: 1}
ROW_S = (511, 512, 513, 1000, 1024, 1025, 2049, 4090, 4096)


def long_rows(S, R=3, seed=None):
    rng = np.random.default_rng(ROW_SEEDS[S] if seed is None else seed)
    ids = ['Row_%d' % g for g in range(R)]
    cov = [mixed_values(rng, S) for _ in range(R)]
    ab = [mixed_values(rng, S) for _ in range(R)]
    reads = [[str(int(v)) for v in rng.integers(0, 10 ** 6, S)] for _ in range(R)]
    order = [[int(g) for g in rng.permutation(R)] for _ in range(S)]
    return ids, cov, ab, reads, profiles_from(ids, cov, ab, reads, order=order)


def row_cases():
    out = []
    for S in ROW_S:
        ids, cov, ab, _, profiles = long_rows(S)
        n_pow2 = 2
        while n_pow2 < S:
            n_pow2 *= 2
        out.append(case('rows/%d' % S, ids, profiles, 'the LDS sort at n_pow2 = %d, a pairwise sum over %d values' % (n_pow2, S), cov_texts=cov, ab_texts=ab))
    return out


def switch_cases():
    out = []
    for S, forms in ((4096, [({}, True), (dict(lds_bound=4095), False)]), (4097, [({}, False)])):
        ids, cov, ab, _, profiles = long_rows(S, seed=ROW_SEEDS[S] + (1000 if S == 4096 else 0))
        out.append(case('switch/default_%d' % S, ids, profiles, 'the default bound of 4096 samples', forms=forms, cov_texts=cov, ab_texts=ab))
    ids, _, _, _, profiles = long_rows(9, R=12, seed=9)
    out.append(case('switch/bound_S_and_S-1', ids, profiles, 'lds_bound = S and S - 1', forms=[(dict(lds_bound=9), True), (dict(lds_bound=8), False)]))
    for R, S in ((1, 2), (2, 3), (3, 2), (4, 5), (5, 4)):
        ids, _, _, _, profiles = long_rows(S, R=R, seed=100 * R + S)
        row_bits = 1
        while (1 << row_bits) < R:
            row_bits += 1
        out.append(case('switch/%d_species_%d_samples' % (R, S), ids, profiles, 'the species pass of the radix sort at row_bits = %d' % row_bits,
                        forms=[(dict(lds_bound=1), False), ({}, True)], row_bits=row_bits))
    return out


# ---- c: designed rows ----------------------------------------------------------------------------------------------------------------
UP1 = '1.0000000000000002'           # nextafter(1.0, 2.0), 17 digits
UP2 = '1.0000000000000004'


def around_middle(S, low, mid_a, mid_b, high):
    """S sorted spellings whose two middle values (the middle one twice over for an odd S) are mid_a <= mid_b."""
    out = [low] * ((S - 1) // 2) + ([mid_a, mid_b] if S % 2 == 0 else [mid_a])
    return out + [high] * (S - len(out))


def designed_rows(S):
    """-> [(what the row is, its S spellings in sorted order)]"""
    half = S // 2
    rows = [
        ('all values equal', ['2.5'] * S),
        ('all -0.0 (eight and nine of them at S = 8 and 9: the leaf starts from r[j] = a[j])', ['-0.0'] * S),
        ('-0.0 and 0.0 around the middle', ['-0.0'] * (S - half) + ['0.0'] * half),
        ('0.0 below -0.0 in file order', ['0.0'] * (S - half) + ['-0.0'] * half),
        ('all negative', ['-%d.25' % (S - k) for k in range(S)]),
        ('the middle pair straddles zero', ['-%d.5' % (half - k) for k in range(half)] + ['%d.25' % (k + 1) for k in range(S - half)]),
        ('ties across the middle', around_middle(S, '0.5', '0.75', '0.75', '0.75') if S < 4 else ['0.5'] * ((S - 1) // 2 - 1) + ['0.75'] * 4 + ['3.0'] * (S - (S - 1) // 2 - 3)),
        ('a middle pair whose sum is inexact', around_middle(S, '0.5', '1.0', UP1, '3.0')),
        ('a middle pair that overflows', around_middle(S, '1.0', '1e308', '1.7e308', '1.75e308')),
        ('values that differ in the low word only', [('1.0', UP1, UP2)[(3 * k) // S] for k in range(S)]),
        ('values that differ in the high word only', sorted(['-1.0', '0.5', '1.0', '1.5', '2.0', '-2.0', '0.25'][k % 7] for k in range(S))),
        ('subnormals', sorted((['5e-324', '1e-320', '0.0', '-5e-324'][k % 4] for k in range(S)), key=float)),
    ]
    for _, r in rows:
        assert len(r) == S
    return rows


def designed_case(S):
    rows = designed_rows(S)
    R = len(rows)
    ids = ['Designed_%02d' % g for g in range(R)]
    place = [(5 * k + 3) % S for k in range(S)]                 # (5 is prime to every S used: a permutation)
    assert sorted(place) == list(range(S))
    cov = [[rows[g][1][place[s]] for s in range(S)] for g in range(R)]
    ab = [[rows[(g + 1) % R][1][place[S - 1 - s]] for s in range(S)] for g in range(R)]
    reads = [[str(g * S + s) for s in range(S)] for g in range(R)]
    order = [[(g + s) % R for g in range(R)] for s in range(S)]
    return case('rowsof/%d' % S, ids, profiles_from(ids, cov, ab, reads, order=order), 'designed rows of %d samples' % S, forms=both_forms(S),
                designed=[w for w, _ in rows], cov_texts=cov, ab_texts=ab)


# ---- d: rounding ---------------------------------------------------------------------------------------------------------------------
ROUND_VALUES = ['0.125', '0.375', '2.675', '1.005', '0.005', '-0.005', '-0.004', '0.285', '1e307', '123456.785', '0.0', '-0.0']


def round_case():
    R = len(ROUND_VALUES)
    ids = ['Round_%02d' % g for g in range(R)]
    cov = [[v] for v in ROUND_VALUES]
    ab = [[ROUND_VALUES[(g + 5) % R]] for g in range(R)]
    reads = [[str(g)] for g in range(R)]
    return case('round/halves', ids, profiles_from(ids, cov, ab, reads), 'rint(x * 100) / 100 on halves, -0.0 and inf as str spells them')


# ---- e: prevalence and order --------------------------------------------------------------------------------------------------------------
DEPTHS = (0.0, 0.5, 1.0, -2.5, math.inf)


def prevalence_case(S, depth):
    """Species k has `counts[k]` coverages exactly on the depth (alternately -0.0 and 0.0 at depth 0.0), the others one ulp below it.
    depth = inf: no finite coverage reaches it, every prevalence is 0."""
    counts = [S // 2, 0, S, max(S - 1, 0), S // 2, min(1, S), 0, S, S // 2, (S + 1) // 2]
    R = len(counts)
    ids = ['Prev_%02d' % g for g in range(R)]
    if math.isinf(depth):
        on, under = ['1.7976931348623157e+308'], '1e308'
    else:
        on = ['0.0', '-0.0'] if depth == 0.0 else [repr(depth)]
        under = repr(float(np.nextafter(np.float64(depth), -np.inf)))
    cov = []
    for g, n in enumerate(counts):
        hit = set((7 * k + g) % S for k in range(n))                # (7 is prime to every S used)
        cov.append([on[s % len(on)] if s in hit else under for s in range(S)])
    rng = np.random.default_rng(1000 + S)
    ab = [M.palette(rng, S) for _ in range(R)]
    reads = [[str(g + s) for s in range(S)] for g in range(R)]
    order = [[(3 * g + s) % R for g in range(R)] for s in range(S)]
    s_bits = 1
    while (1 << s_bits) <= S:
        s_bits += 1
    return case('prev/%d_samples_depth_%r' % (S, depth), ids, profiles_from(ids, cov, ab, reads, order=order),
                'prevalence 0 and %d, the order key on %d bits, coverages on and one ulp under %r' % (S, s_bits, depth), sample_depth=depth, forms=both_forms(S),
                counts=[0] * R if math.isinf(depth) else counts)


# ---- f: the lookup table -----------------------------------------------------------------------------------------------------------------
CANDIDATES = ['Sp_%04d' % k for k in range(2000)]


def homed(slot, size, skip=()):
    return [c for c in CANDIDATES if home(c, size) == slot and c not in skip]


def plain_profiles(ids, S=2, seed=7, **kw):
    rng = np.random.default_rng(seed)
    R = len(ids)
    cov, ab = [M.palette(rng, S) for _ in range(R)], [M.palette(rng, S) for _ in range(R)]
    reads = [[str(int(v)) for v in rng.integers(0, 10 ** 6, S)] for _ in range(R)]
    order = [[int(g) for g in rng.permutation(R)] for _ in range(S)]
    return profiles_from(ids, cov, ab, reads, order=order, **kw)


def with_line_for(profiles, ids, victim, intruder, sample=1):
    """The line of species `victim` in one sample names `intruder` instead."""
    out = list(profiles)
    assert out[sample].count('\n' + ids[victim] + '\t') == 1
    out[sample] = out[sample].replace('\n' + ids[victim] + '\t', '\n' + intruder + '\t')
    return out


def table_cases():
    out = []
    # one chain of seven: every id hashes to slot 4 of 16
    full = homed(4, 16)[:7]
    stranger = homed(4, 16)[7]
    out.append(case('table/seven_in_one_slot', full, plain_profiles(full), 'a probe chain of seven slots', chain=list(range(4, 11))))
    out.append(case('table/refused_head_of_the_full_chain', full, with_line_for(plain_profiles(full), full, 3, stranger),
                    'an unknown id down the whole chain to the empty slot behind it', refused=True, intruder=stranger, visits=list(range(4, 12))))
    # a chain from the last slot over slot 0
    last, zero = homed(15, 16), homed(0, 16)
    wrapped = last[:3] + zero[:1] + [homed(k, 16)[0] for k in (6, 7, 8)]
    out.append(case('table/wraps_to_slot_0', wrapped, plain_profiles(wrapped), 'a chain over the last slot and slot 0', chain=[15, 0, 1, 2, 6, 7, 8]))
    out.append(case('table/refused_in_the_wrapped_chain', wrapped, with_line_for(plain_profiles(wrapped), wrapped, 5, last[3]),
                    'an unknown id from the last slot over slot 0 to an empty one', refused=True, intruder=last[3], visits=[15, 0, 1, 2, 3]))
    # the growth borders, one id with bytes above 0x7F
    for R in (7, 8, 15, 16):
        ids = ['Sp\u00e9\u4e2d_%d' % R] + CANDIDATES[100:100 + R - 1]
        out.append(case('table/%d_ids' % R, ids, plain_profiles(ids, seed=R), '%d ids in %d slots' % (R, table_size(R)), size=table_size(R)))
    # near misses of a known id, in the slot of a known id
    ids = CANDIDATES[100:108]
    size = table_size(len(ids))
    occupied = set(table_of(ids)[2])
    near = {}
    for g, known in enumerate(ids):
        k = home(known, size)
        for c in '0123456789abcdefghijklmnopqrstuvwxyz':
            if c != known[-1] and home(known[:-1] + c, size) == k and known[:-1] + c not in ids:
                near.setdefault('last_byte', (g, known[:-1] + c))
            if c != known[0] and home(c + known[1:], size) == k:
                near.setdefault('first_byte', (g, c + known[1:]))
            if home(known + c, size) in occupied:
                near.setdefault('extension', (g, known + c))
        for cut in range(1, len(known)):
            if home(known[:cut], size) in occupied:
                near.setdefault('prefix', (g, known[:cut]))
    near['empty'] = (2, '')
    for kind in ('last_byte', 'first_byte', 'prefix', 'extension', 'empty'):
        g, intruder = near[kind]
        out.append(case('table/refused_%s' % kind, ids, with_line_for(plain_profiles(ids, seed=3), ids, g, intruder),
                        {'last_byte': 'an id equal to a known one but for its last byte, in its slot', 'first_byte': 'an id equal to a known one but for its first byte, in its slot',
                         'prefix': 'a proper prefix of a known id', 'extension': 'a known id and one byte more', 'empty': 'the empty id'}[kind],
                        refused=True, intruder=intruder, near=ids[g], kind=kind))
    return out


# ---- g: the field splitter -----------------------------------------------------------------------------------------------------------------
WIDE = ['note'] + list(M.COLUMNS) + ['tail']


def residue_profiles():
    """Two samples under the header note | the four columns | tail: row g opens with a cell of g % 37 bytes, so the lines start, the
    tabs fall and the lines end on every residue of the 16-byte words."""
    R = 96
    ids = ['R%d' % g if g % 3 else 'Residue_%03d' % g for g in range(R)]
    rng = np.random.default_rng(16)
    cov, ab = [M.palette(rng, 2) for _ in range(R)], [M.palette(rng, 2) for _ in range(R)]
    reads = [[str(int(v)) for v in rng.integers(0, 10 ** int(rng.integers(1, 9)), 2)] for _ in range(R)]
    filler = lambda name, f, g, s: ('n' * ((g + 5 * s) % 37)) if name == 'note' else ('t' * ((g * 7 + s) % 5))
    order = [list(range(R)), list(range(R - 1, -1, -1))]
    return ids, profiles_from(ids, cov, ab, reads, order=order, header=WIDE, extra_columns=filler)


def residues(text, offset, header=None):
    """Where the fields kernel meets a profile that stands at `offset` of its group's text -> {what: set of residues mod 16} over the
    live lines: 'start', 'end' (the newline), and per named column the tab that closes it."""
    lines = text.split('\n')
    fields = lines[0].split('\t')
    out = dict(start=set(), end=set())
    for c in M.COLUMNS:
        out[c] = set()
    at = offset + len(lines[0].encode()) + 1
    for line in lines[1:]:
        n = len(line.encode())
        cells = line.split('\t')
        if len(cells) == len(fields):
            out['start'].add(at % 16)
            out['end'].add((at + n) % 16)
            pos = at
            for name, cell in zip(fields, cells):
                pos += len(cell.encode())
                if name in out and pos < at + n:
                    out[name].add(pos % 16)
                pos += 1
        at += n + 1
    return out


def forty_columns(reverse):
    named = dict(zip((0, 17, 38, 39), M.COLUMNS[::-1] if reverse else M.COLUMNS))
    return [named.get(f, 'c%02d' % f) for f in range(40)]


GOOD_IDS = ['a', 'bb', 'ccc']
GOOD = HEAD + 'a\t1\t1.5\t0.5\nbb\t2\t2.5\t0.25\nccc\t3\t0.0\t0.25\n'
CHUNKS = [(dict(chunk_bytes=0), True), (dict(chunk_bytes=16), True)]


def field_cases():
    out = []
    ids, profiles = residue_profiles()
    out.append(case('fields/sixteen_residues', ids, profiles, 'line starts, line ends and closing tabs on every residue of a 16-byte word', forms=CHUNKS))
    rng = np.random.default_rng(40)
    ids = ['Wide_%d' % g for g in range(5)]
    cov, ab = [M.palette(rng, 2) for _ in ids], [M.palette(rng, 2) for _ in ids]
    reads = [[str(g), str(10 * g)] for g in range(5)]
    filler = lambda name, f, g, s: '%d.%d' % (f, g) if f % 3 else ''
    wide = [profiles_from(ids, cov, ab, reads, header=forty_columns(False), extra_columns=filler)[0],
            profiles_from(ids, cov, ab, reads, header=forty_columns(True), extra_columns=filler)[1]]
    out.append(case('fields/forty_columns', ids, wide, 'named columns at fields 0, 17, 38, 39 and in the opposite order; empty unnamed cells', forms=CHUNKS))
    ids = GOOD_IDS
    accept = [
        ('dropped_lines', GOOD.replace('bb\t2', 'a\t1\t1.5\t0.5\t9\nbb\t2\t2.5\n\t\t\n\t\t\t\t\nbb\t2'), 'one field more, one fewer, tabs alone: dropped'),
        ('int64_ends', GOOD.replace('\t1\t', '\t9223372036854775807\t').replace('\t2\t', '\t-9223372036854775808\t'), 'count_reads at both ends of int64, by the side list'),
        ('no_final_newline', GOOD[:-1], 'a profile that does not end in a newline'),
        ('crlf_unnamed_last', GOOD.replace('\n', '\tz\r\n'), 'CRLF behind an unnamed last column'),
        ('lookalike_headers', profiles_from(GOOD_IDS, [['1.5'], ['2.5'], ['0.0']], [['0.5'], ['0.25'], ['0.25']], [['1'], ['2'], ['3']],
                                            header=['coverage2', ' species_id', 'Coverage'] + list(M.COLUMNS),
                                            extra_columns=lambda name, f, g, s: {'coverage2': '9.5', ' species_id': 'q', 'Coverage': '8.5'}[name])[0],
         "header cells that only start with or resemble a column's name, beside the real ones"),
    ]
    for name, text, on in accept:
        assert text != GOOD
        out.append(case('fields/' + name, ids, [GOOD, text, GOOD], on, forms=CHUNKS, side_cells=name == 'int64_ends'))
    refuse = [
        ('empty_count_reads', GOOD.replace('bb\t2\t', 'bb\t\t'), 7), ('empty_coverage', GOOD.replace('\t2.5\t', '\t\t'), 8),
        ('count_reads_plus', GOOD.replace('\t3\t', '\t+\t'), 7), ('count_reads_minus', GOOD.replace('\t3\t', '\t-\t'), 7),
        ('count_reads_1.0', GOOD.replace('\t3\t', '\t1.0\t'), 7),
        ('header_alone', HEAD[:-1], M.MISSING),
        ('crlf_named_last', GOOD.replace('\n', '\r\n'), 4),
        ('coverage2_for_coverage', GOOD.replace('coverage', 'coverage2'), 3), ('blank_species_id', GOOD.replace('species_id', ' species_id'), 1),
        ('Coverage_for_coverage', GOOD.replace('coverage', 'Coverage'), 3),
    ]
    for name, text, reason in refuse:
        assert text != GOOD
        out.append(case('fields/refused_' + name, ids, [GOOD, text, GOOD.replace('a\t1', 'q\t1')], 'refused for reason %d' % reason, forms=CHUNKS, refused=True, reason=reason))
    return out


# ---- h: the writer ---------------------------------------------------------------------------------------------------------------------
def writer_case(R=130, S=2048):
    """Row blocks of 65536 // S rows, formatted in waves of 4 * threads blocks: five blocks, so two waves of one thread."""
    assert R * S > 4 * 65536 and R > 4 * (65536 // S)
    rng = np.random.default_rng(2048)
    pool = np.array(mixed_values(rng, 1009))
    ids = ['Written_%s_%03d' % ('y' * (g % 5), g) for g in range(R)]
    cov, ab = pool[rng.integers(0, len(pool), (R, S))], pool[rng.integers(0, len(pool), (R, S))]
    reads = rng.integers(-10 ** 6, 10 ** 12, (R, S)).astype(str)
    profiles = []
    for s in range(S):
        profiles.append(HEAD + ''.join('%s\t%s\t%s\t%s\n' % (ids[g], reads[g, s], cov[g, s], ab[g, s]) for g in range(R)))
    return case('write/five_blocks', ids, profiles, '%d blocks of %d rows: two waves with one thread, one wave with two' % (-(-R // (65536 // S)), 65536 // S),
                write_threads=(1, 2), blocks=-(-R // (65536 // S)))


# ---- all of them -----------------------------------------------------------------------------------------------------------------------
PREV_S = (1, 2, 4, 8, 128, 256)
DESIGNED_S = (1, 2, 3, 4, 8, 9, 16, 17)
_cache = {}


def cases(family):
    """The cases of a family, built once."""
    if family not in _cache:
        _cache[family] = {'rows': row_cases, 'switch': switch_cases, 'rowsof': lambda: [designed_case(S) for S in DESIGNED_S], 'round': lambda: [round_case()],
                          'prev': lambda: [prevalence_case(S, d) for S in PREV_S for d in DEPTHS], 'table': table_cases, 'fields': field_cases,
                          'write': lambda: [writer_case()]}[family]()
    return _cache[family]


FAMILIES = ('rows', 'switch', 'rowsof', 'round', 'prev', 'table', 'fields', 'write')
_expect = {}


def expect(c):
    """What the model makes of a case, computed once and shared: M.merge's dict, or for a refusal M.first_error's BadProfile."""
    if c['name'] not in _expect:
        _expect[c['name']] = M.first_error(c['profiles'], c['ids']) if c['refused'] else M.merge(c['sample_ids'], c['profiles'], c['ids'], c['sample_depth'])
    return _expect[c['name']]


def names(family):
    return [c['name'] for c in cases(family)]


def named(name):
    return [c for c in cases(name.split('/')[0]) if c['name'] == name][0]
