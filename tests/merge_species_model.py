"""A sequential restatement of merge_species.py with plain np.mean, np.median, round and str: what midas/merge/species.py computes
from the samples' species profiles, plus the checks this build adds.  Held to every case of tests/golden/merge_species_vectors.json
(recorded from the reference's own functions), then used as the expectation of the larger random cases of the GPU tests."""
import json
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FILES = ('relative_abundance.txt', 'coverage.txt', 'count_reads.txt', 'species_prevalence.txt')
COLUMNS = ('species_id', 'count_reads', 'coverage', 'relative_abundance')
# the reasons of midas_species_merge (include/midas_snps.h)
HEADER, UNKNOWN, TWICE, CELL, NON_FINITE, RANGE, MISSING = 1, 5, 6, 7, 10, 12, 13
CELL_OF = {'count_reads': 7, 'coverage': 8, 'relative_abundance': 9}
NON_FINITE_OF = {'coverage': 10, 'relative_abundance': 11}


class BadProfile(Exception):
    def __init__(self, reason, sample, line, what):
        Exception.__init__(self, "sample %d line %d: reason %d (%s)" % (sample, line, reason, what))
        self.reason, self.sample, self.line, self.what = reason, sample, line, what


def load_vectors():
    with open(os.path.join(HERE, 'golden', 'merge_species_vectors.json')) as handle:
        return json.load(handle)


def species_ids(species_info):
    lines = species_info.split('\n')
    fields = lines[0].split('\t')
    ids = {}
    for line in lines[1:]:
        values = line.split('\t')
        if len(values) == len(fields):
            ids[dict(zip(fields, values))['species_id']] = None
    return list(ids)


def identify_samples(indirs, has_profile, max_samples=None):
    """-> (the directories kept, what goes to stderr); has_profile(dir) says whether species/species_profile.txt exists."""
    kept, err = [], ''
    for d in indirs:
        if not has_profile(d):
            err += "Warning: missing/incomplete output: %s\n" % d
        elif os.path.basename(d) in [os.path.basename(k) for k in kept]:
            err += "Warning: sample_id '%s' specified more than one time.\nSkipping: %s\n" % (os.path.basename(d), d)
        else:
            kept.append(d)
    if max_samples is not None and len(kept) > max_samples:
        kept = kept[0:max_samples]
    return kept, err


def read_profile(text, ids, sample=0):
    """utility.parse_file + read_abundance over one profile's text -> {species_id: (count_reads, coverage, relative_abundance)};
    the first line that this build refuses raises BadProfile (a species without a line: the line after the last)."""
    lines = text.split('\n')
    if lines and lines[-1] == '':
        lines.pop()
    fields = lines[0].split('\t') if lines else ['']
    for k, name in enumerate(COLUMNS):
        if name not in fields:
            raise BadProfile(HEADER + k, sample, 1, name)
    known, out = set(ids), {}
    for n, line in enumerate(lines[1:], 2):
        values = line.split('\t')
        if len(values) != len(fields):
            continue
        rec = dict(zip(fields, values))
        bad = []                                        # every refusal of the line; the lowest reason is the one reported
        if rec['species_id'] not in known:
            bad.append((UNKNOWN, rec['species_id']))
        elif rec['species_id'] in out:
            bad.append((TWICE, rec['species_id']))
        row = []
        for name in COLUMNS[1:]:
            try:
                v = int(rec[name]) if name == 'count_reads' else float(rec[name])
            except ValueError:
                bad.append((CELL_OF[name], name))
                v = 0
            if name == 'count_reads' and not -2 ** 63 <= v < 2 ** 63:
                bad.append((RANGE, name))
            if name != 'count_reads' and not math.isfinite(v):
                bad.append((NON_FINITE_OF[name], name))
            row.append(v)
        if bad:
            raise BadProfile(min(bad)[0], sample, n, min(bad)[1])
        out[rec['species_id']] = tuple(row)
    for k, s in enumerate(ids):
        if s not in out:
            raise BadProfile(MISSING, sample, len(lines) + 1, s)
    return out


def merge(sample_ids, profiles, ids, sample_depth):
    """-> dict(files: the four texts, coverage / abundance / reads as lists of rows, mean_coverage ... per species as np.float64,
    rounded, prevalence, order)."""
    data = [read_profile(text, ids, k) for k, text in enumerate(profiles)]
    cov = [[d[s][1] for d in data] for s in ids]
    ab = [[d[s][2] for d in data] for s in ids]
    reads = [[d[s][0] for d in data] for s in ids]
    head = '\t'.join(['species_id'] + list(sample_ids)) + '\n'
    files = {}
    for name, m in (('relative_abundance.txt', ab), ('coverage.txt', cov), ('count_reads.txt', reads)):
        files[name] = head + ''.join(s + ''.join('\t%s' % str(x) for x in row) + '\n' for s, row in zip(ids, m))
    stats = dict(mean_coverage=[np.mean(x) for x in cov], median_coverage=[np.median(x) for x in cov],
                 mean_abundance=[np.mean(x) for x in ab], median_abundance=[np.median(x) for x in ab])
    prevalence = [sum(1 if v >= sample_depth else 0 for v in x) for x in cov]
    order = sorted(range(len(ids)), key=lambda k: prevalence[k], reverse=True)
    names = ['mean_coverage', 'median_coverage', 'mean_abundance', 'median_abundance']
    rounded = dict((n, [round(v, 2) for v in stats[n]]) for n in names)
    text = '\t'.join(['species_id'] + names + ['prevalence']) + '\n'
    for k in order:
        text += ids[k] + ''.join('\t%s' % str(rounded[n][k]) for n in names) + '\t%s\n' % str(prevalence[k])
    files['species_prevalence.txt'] = text
    out = dict(files=files, coverage=cov, abundance=ab, reads=reads, rounded=rounded, prevalence=prevalence, order=order)
    out.update(stats)
    return out


def first_error(profiles, ids):
    """The BadProfile the merge reports (the earliest in the order of samples), or None."""
    for k, text in enumerate(profiles):
        try:
            read_profile(text, ids, k)
        except BadProfile as e:
            return e
    return None


def run_case(vec, case):
    """A golden case through the model -> (files, stderr)."""
    profiles = case['profiles']
    kept, err = identify_samples(case['indirs'], lambda d: profiles.get(d) is not None, case['max_samples'])
    got = merge([os.path.basename(d) for d in kept], [profiles[d] for d in kept], species_ids(vec['species_info']), case['sample_depth'])
    return got['files'], err


def write_case(root, vec, case):
    """The database and the sample directories of a golden case under root -> (db, the input directories)."""
    db = os.path.join(root, 'db')
    os.makedirs(db, exist_ok=True)
    with open(os.path.join(db, 'species_info.txt'), 'w') as handle:
        handle.write(vec['species_info'])
    for d, text in case['profiles'].items():
        os.makedirs(os.path.join(root, d, 'species') if text is not None else os.path.join(root, d), exist_ok=True)
        if text is not None:
            with open(os.path.join(root, d, 'species', 'species_profile.txt'), 'w') as handle:
                handle.write(text)
    return db, [os.path.join(root, d) for d in case['indirs']]


def palette(rng, n):
    """n doubles as repr texts: few and many digits, small and large, exponents, zeros, ties."""
    out = []
    for _ in range(n):
        kind = int(rng.integers(0, 8))
        if kind == 0:
            out.append('0.0')
        elif kind == 1:
            out.append(repr(round(float(rng.random()) * 10.0, 2)))
        elif kind == 2:
            out.append(repr(float(rng.random()) * 10.0 ** int(rng.integers(-6, 5))))       # 16-17 digits: the host's parser
        elif kind == 3:
            out.append(repr(float(rng.integers(0, 5))))
        elif kind == 4:
            out.append(repr(float(rng.integers(1, 10 ** 6)) / 1000.0))
        elif kind == 5:
            out.append('%de-%d' % (int(rng.integers(1, 10 ** 5)), int(rng.integers(1, 9))))
        else:
            out.append(repr(round(float(rng.random()) * 3.0, int(rng.integers(1, 9)))))
    return out


def synth(n_species, n_samples, seed, shuffle=True):
    """-> (species ids, sample ids, profile texts): every species in every profile, rows in a random order per sample."""
    rng = np.random.default_rng(seed)
    ids = ['Species_%s_%05d' % ('x' * (k % 7), k) for k in range(n_species)]
    sample_ids = ['sample_%04d' % s for s in range(n_samples)]
    profiles = []
    for s in range(n_samples):
        cov, ab = palette(rng, n_species), palette(rng, n_species)
        reads = rng.integers(0, 10 ** 6, n_species)
        rows = ['%s\t%d\t%s\t%s' % (ids[k], reads[k], cov[k], ab[k]) for k in (rng.permutation(n_species) if shuffle else range(n_species))]
        profiles.append('species_id\tcount_reads\tcoverage\trelative_abundance\n' + '\n'.join(rows) + '\n')
    return ids, sample_ids, profiles


def write_samples(root, sample_ids, profiles):
    """-> the profile paths, sample directories under root."""
    paths = []
    for s, text in zip(sample_ids, profiles):
        os.makedirs(os.path.join(root, s, 'species'), exist_ok=True)
        paths.append(os.path.join(root, s, 'species', 'species_profile.txt'))
        with open(paths[-1], 'w') as handle:
            handle.write(text)
    return paths


if __name__ == '__main__':
    vec = load_vectors()
    for case in vec['cases']:
        files, err = run_case(vec, case)
        assert files == case['outputs'] and err == case['stderr'], case['name']
    print("%d cases" % len(vec['cases']), file=sys.stderr)
