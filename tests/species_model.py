"""A sequential model of run_species.py's classify step (what midas/run/species.py:51-175 computes), written from its
description: line by line, one query after another, with its own MT19937.  The tests hold the device, the native chain and the
command-line tool against it, and hold it against vectors recorded from the reference's own functions
(tests/golden/species_vectors.json)."""

import os


class MT19937:
    """The generator behind random and numpy's legacy global state: 624 words and a position."""

    def __init__(self, words, pos):
        self.mt = [int(w) for w in words]
        self.pos = int(pos)
        assert len(self.mt) == 624

    def word(self):
        mt = self.mt
        if self.pos >= 624:
            for k in range(624):
                y = (mt[k] & 0x80000000) | (mt[(k + 1) % 624] & 0x7FFFFFFF)
                mt[k] = mt[(k + 397) % 624] ^ (y >> 1) ^ (0x9908B0DF if y & 1 else 0)
            self.pos = 0
        y = mt[self.pos]
        self.pos += 1
        y ^= y >> 11
        y ^= (y << 7) & 0x9D2C5680
        y ^= (y << 15) & 0xEFC60000
        y ^= y >> 18
        return y & 0xFFFFFFFF

    def below(self, k):
        """random's index below k: getrandbits(k.bit_length()) until it is one."""
        bits = k.bit_length()
        while True:
            r = self.word() >> (32 - bits)
            if r < k:
                return r

    def double(self):
        """numpy's legacy random_sample(): 53 bits of two words."""
        a, b = self.word() >> 5, self.word() >> 6
        return (a * 67108864.0 + b) / 9007199254740992.0


def generators(seed=None, py_state=None, np_state=None):
    """The two generators as random.seed(seed) / np.random.seed(seed) leave them (or from the given states)."""
    import random
    import numpy as np
    if seed is not None:
        r = random.Random(seed)
        py_state = r.getstate()
        np_state = np.random.RandomState(seed).get_state()
    return MT19937(py_state[1][:624], py_state[1][624]), MT19937(np_state[1], np_state[2])


class Database:
    """species_info.txt, marker_genes/phyeco.{fa,map,mapping_cutoffs} as the classify step uses them."""

    def __init__(self, species, genes, cutoffs):
        self.species = list(species)                        # ids in species_info.txt order
        self.genes = dict(genes)                            # gene_id -> (species_id, marker_id, gene_length); phyeco.fa genes only
        self.cutoffs = dict(cutoffs)                        # marker_id -> float

    @classmethod
    def read(cls, db):
        def table(path):
            with open(path) as handle:
                fields = next(handle).rstrip('\n').split('\t')
                for line in handle:
                    values = line.rstrip('\n').split('\t')
                    if len(values) == len(fields):
                        yield dict(zip(fields, values))
        species = list(dict.fromkeys(r['species_id'] for r in table(os.path.join(db, 'species_info.txt'))))
        in_fa = {}
        with open(os.path.join(db, 'marker_genes', 'phyeco.fa')) as handle:
            for line in handle:
                if line.startswith('>'):
                    in_fa[line[1:].split()[0]] = None
        for r in table(os.path.join(db, 'marker_genes', 'phyeco.map')):
            if r['gene_id'] in in_fa:
                in_fa[r['gene_id']] = (r['species_id'], r['marker_id'], int(r['gene_length']))
        cutoffs = {}
        with open(os.path.join(db, 'marker_genes', 'phyeco.mapping_cutoffs')) as handle:
            for line in handle:
                marker_id, min_pid = line.rstrip().split()
                cutoffs[marker_id] = float(min_pid)
        return cls(species, in_fa, cutoffs)


class BadLine(Exception):
    def __init__(self, line, reason):
        Exception.__init__(self, "line %d: %s" % (line, reason))
        self.line, self.reason = line, reason


def parse_lines(text, db, mapid=None, aln_cov=0.75):
    """Every line decoded and filtered -> list of dict(query, species, marker, pid, aln, qlen, score, passed).  The first bad
    line raises BadLine(1-based line, reason): 'fields', 'target', 'qlen', 'aln', 'number'."""
    out = []
    lines = text.split('\n')
    if lines and lines[-1] == '':
        lines.pop()
    for number, line in enumerate(lines, 1):
        values = line.split()
        if len(values) < 12:
            raise BadLine(number, 'fields')
        query, target = values[0], values[1]
        gene = db.genes.get(target)
        if gene is None:
            raise BadLine(number, 'target')
        try:
            pid, score = float(values[2]), float(values[11])
        except ValueError:
            raise BadLine(number, 'number')
        try:
            aln = int(values[3])
        except ValueError:
            raise BadLine(number, 'aln')
        try:
            qlen = int(query.split('_')[-1])
        except ValueError:
            raise BadLine(number, 'qlen')
        if qlen == 0:
            raise BadLine(number, 'qlen')
        cutoff = mapid if mapid else db.cutoffs[gene[1]]
        passed = not (pid < cutoff) and not (float(aln) / qlen < aln_cov)
        out.append(dict(query=query, species=gene[0], marker=gene[1], pid=pid, aln=aln, qlen=qlen, score=score, passed=passed))
    return out


def best_hits(rows):
    """Per query, in the order of its first passing line, the passing lines whose score is the query's maximum, in line order."""
    top = {}
    for r in rows:
        if r['passed']:
            top[r['query']] = max(top.get(r['query'], r['score']), r['score'])
    hits = {}
    for r in rows:
        if r['passed']:
            hits.setdefault(r['query'], [])
            if r['score'] == top[r['query']]:
                hits[r['query']].append(r)
    return list(hits.values())


def assign(hits, species, py, nprng, frozen=False):
    """-> ({species: reads}, {species: aln sum}, unique queries, ambiguous queries).  frozen: the weights of a draw are the
    unique reads alone (NOT what the reference does: the tests use it to show that the vectors pin the chain)."""
    reads = dict((s, 0) for s in species)
    bases = dict((s, 0) for s in species)
    unique = 0
    for h in hits:
        if len(h) == 1:
            unique += 1
            reads[h[0]['species']] += 1
            bases[h[0]['species']] += h[0]['aln']
    weights = dict(reads) if frozen else reads
    for h in hits:
        if len(h) < 2:
            continue
        ids = [x['species'] for x in h]
        pick = draw([weights[i] for i in ids], py, nprng)
        first = ids.index(ids[pick])
        reads[ids[pick]] += 1
        bases[ids[pick]] += h[first]['aln']
    return reads, bases, unique, len(hits) - unique


def draw(counts, py, nprng):
    """The index of the hit a read with these per-hit species counts goes to."""
    total = sum(counts)
    if total == 0:
        return py.below(len(counts))
    run, cdf = 0.0, []
    for c in counts:
        run += float(c) / total
        cdf.append(run)
    u = nprng.double()
    return sum(1 for x in cdf if x / cdf[-1] <= u)


def profile_text(db, reads, bases):
    """species_profile.txt and the total coverage."""
    length = dict((s, 0) for s in db.species)
    for gene in db.genes.values():
        if gene is not None:
            length[gene[0]] += gene[2]
    cov = dict((s, float(bases[s]) / length[s] if reads[s] > 0 else 0.0) for s in db.species)
    total = sum([cov[s] for s in db.species])
    rows = ['\t'.join(['species_id', 'count_reads', 'coverage', 'relative_abundance'])]
    for s in sorted(db.species, key=lambda s: reads[s], reverse=True):
        rows.append('\t'.join(str(x) for x in (s, reads[s], cov[s], cov[s] / total if total > 0 else 0)))
    return '\n'.join(rows) + '\n', total


def classify(text, db, seed=None, mapid=None, aln_cov=0.75, frozen=False, py_state=None, np_state=None):
    """-> dict(profile, printed, rows, hits, reads, bases): the whole step."""
    rows = parse_lines(text, db, mapid, aln_cov)
    hits = best_hits(rows)
    py, nprng = generators(seed, py_state, np_state)
    reads, bases, unique, ambiguous = assign(hits, db.species, py, nprng, frozen)
    profile, total = profile_text(db, reads, bases)
    printed = ["  total alignments: %s" % len(rows), "  uniquely mapped reads: %s" % unique, "  ambiguously mapped reads: %s" % ambiguous,
               "  total marker-gene coverage: %s" % round(total, 3)]
    return dict(profile=profile, printed=printed, rows=rows, hits=hits, reads=reads, bases=bases)


def csr(hits, species):
    """The ambiguous queries as (indptr, species index, aln) lists and the unique reads' per-species (reads, aln)."""
    index = dict((s, k) for k, s in enumerate(species))
    indptr, sp, aln = [0], [], []
    reads, bases = [0] * len(species), [0] * len(species)
    for h in hits:
        if len(h) == 1:
            reads[index[h[0]['species']]] += 1
            bases[index[h[0]['species']]] += h[0]['aln']
        else:
            sp += [index[x['species']] for x in h]
            aln += [x['aln'] for x in h]
            indptr.append(len(sp))
    return indptr, sp, aln, reads, bases


def load_vectors():
    import json
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'species_vectors.json')) as handle:
        return json.load(handle)


def write_db(db, files, genomes=()):
    """The golden database as a MIDAS database directory (with the pieces check_database asks for; `genomes`: species that get
    a small representative genome)."""
    for sub in ('marker_genes', 'pan_genomes', 'rep_genomes'):
        os.makedirs(os.path.join(db, sub), exist_ok=True)
    for name, key in (('species_info.txt', 'species_info'), ('marker_genes/phyeco.fa', 'phyeco_fa'), ('marker_genes/phyeco.map', 'phyeco_map'),
                      ('marker_genes/phyeco.mapping_cutoffs', 'phyeco_mapping_cutoffs')):
        with open(os.path.join(db, name), 'w') as handle:
            handle.write(files[key])
    with open(os.path.join(db, 'genome_info.txt'), 'w') as handle:
        handle.write('genome_id\tspecies_id\n')
    for s in genomes:
        os.makedirs(os.path.join(db, 'rep_genomes', s), exist_ok=True)
        with open(os.path.join(db, 'rep_genomes', s, 'genome.fna'), 'w') as handle:
            handle.write('>%s_contig\nACGTACGTACGTTTGACA\n' % s)
    return db


def write_sample(out, m8):
    os.makedirs(os.path.join(out, 'species', 'temp'), exist_ok=True)
    with open(os.path.join(out, 'species', 'temp', 'alignments.m8'), 'w') as handle:
        handle.write(m8)
    return out


def synth_m8(n_queries, n_species, n_markers, seed, shuffle=False):
    """A synthetic database (as Database) and m8 text: reads named r<k>_<len> with one to eight lines, scores from a few levels
    so that ties are common, every spelling class of pid / score, some lines failing each filter."""
    import numpy as np
    rng = np.random.default_rng(seed)
    species = ['S%04d' % k for k in range(n_species)]
    markers = ['B%06d' % (k + 1) for k in range(n_markers)]
    genes = {}
    names = []
    for k, s in enumerate(species):
        for m, marker in enumerate(markers):
            g = '%d.%d.peg.%d' % (10000 + k, 1 + k % 3, 5 + 3 * m)
            genes[g] = (s, marker, int(rng.integers(300, 2000)))
            names.append(g)
    cutoffs = dict((marker, 94.0 + 0.25 * (m % 16)) for m, marker in enumerate(markers))
    lines = []
    hot = rng.integers(0, n_species, size=max(2, n_species // 4))
    for q in range(n_queries):
        qlen = int(rng.choice([75, 100, 101, 150, 250]))
        name = 'r%d_%d' % (q, qlen) if q % 7 else 'lib_%d/r%d_%d' % (q % 3, q, qlen)
        top = float(rng.choice([90.5, 120.0, 150.0, 187.0]))
        for j in range(int(rng.choice([1, 2, 3, 4, 4, 5, 8]))):
            s = int(rng.choice(hot)) if rng.random() < 0.7 else int(rng.integers(0, n_species))
            g = names[s * n_markers + int(rng.integers(0, n_markers))]
            score = top if rng.random() < 0.7 else top - float(rng.integers(1, 40)) / 2
            pid = float(rng.choice([93.0, 95.0, 96.5, 98.25, 99.0, 100.0])) + int(rng.integers(0, 100)) / 100
            aln = int(qlen * float(rng.choice([0.5, 0.74, 0.75, 0.76, 1.0])))
            r = rng.random()
            if r < 0.03:
                spid, sscore = repr(pid + 1e-13), '%.1e' % score if score == 120.0 else repr(score)        # 16-17 digits; 1.2e+02
            elif r < 0.06:
                spid, sscore = '%.2f' % pid, '%de-1' % int(score * 10)
            elif r < 0.08:
                spid, sscore = '+%s' % pid, '%s0000000000000000' % score                                 # more than 15 digits
            else:
                spid, sscore = '%.2f' % pid, str(score)
            sep = '\t' if r > 0.02 else ' \t  '
            lines.append(sep.join([name, g, spid, str(aln), '2', '0', '1', str(aln), '11', str(10 + aln), '3e-40', sscore]))
    if shuffle:
        lines = [lines[i] for i in rng.permutation(len(lines))]
    return Database(species, genes, cutoffs), '\n'.join(lines) + '\n'
