"""run_species.py: reads -> hs-blastn against the marker genes -> species_profile.txt (what midas/run/species.py computes).

The align stage streams the reads as `>id_length` FASTA records into hs-blastn (from PATH; no binary ships here).  The classify
stage is the library's: the m8 lines are parsed, filtered, grouped by query and reduced to best hits on the device
(abi.Context.species_classify), the reads whose best hits tie are given out by the serial chain on the host
(abi.species_assign, with the interpreter's two generator states), and the table -- a few thousand numbers -- is written here.
"""

import os
import shutil
import subprocess
import sys
from time import time

import numpy as np

from midas_amd import utility


def _table(path):
    """utility.parse_file of the reference: tab separated with a header, rows of another width skipped."""
    with utility.iopen(path) as handle:
        fields = next(handle).rstrip('\n').split('\t')
        for line in handle:
            values = line.rstrip('\n').split('\t')
            if len(values) == len(fields):
                yield dict(zip(fields, values))


class MarkerDatabase:
    """species_info.txt and marker_genes/phyeco.{fa,map,mapping_cutoffs} as arrays for the device."""

    def __init__(self, db, mapid=None):
        self.species = list(dict.fromkeys(r['species_id'] for r in _table(os.path.join(db, 'species_info.txt'))))
        index = dict((s, k) for k, s in enumerate(self.species))
        in_fa = {}
        with utility.iopen(os.path.join(db, 'marker_genes', 'phyeco.fa')) as handle:
            for line in handle:
                if line.startswith('>'):
                    in_fa[line[1:].split()[0]] = None
        for r in _table(os.path.join(db, 'marker_genes', 'phyeco.map')):
            if r['gene_id'] in in_fa:
                in_fa[r['gene_id']] = r
        cutoffs_path = os.path.join(db, 'marker_genes', 'phyeco.mapping_cutoffs')
        if not os.path.isfile(cutoffs_path):
            sys.exit("File not found: %s" % cutoffs_path)
        cutoffs = {}
        with open(cutoffs_path) as handle:
            for line in handle:
                marker_id, min_pid = line.rstrip().split()
                cutoffs[marker_id] = mapid if mapid else float(min_pid)
        rows = [(g, r) for g, r in in_fa.items() if r is not None]      # a gene without a map row: a hit on it is an error
        self.markers = list(dict.fromkeys(r['marker_id'] for _, r in rows))
        marker_index = dict((m, k) for k, m in enumerate(self.markers))
        self.gene_names = [g.encode() for g, _ in rows]
        for _, r in rows:
            if r['species_id'] not in index:
                sys.exit("\nError: marker gene %s belongs to species %s, which species_info.txt does not list\n" % (r['gene_id'], r['species_id']))
        self.gene_species = np.array([index[r['species_id']] for _, r in rows], np.int32)
        self.gene_marker = np.array([marker_index[r['marker_id']] for _, r in rows], np.int32)
        # (a family without a cutoff: nan, an error at the first hit on it -- the reference's KeyError)
        self.cutoff = np.array([mapid if mapid else cutoffs.get(m, float('nan')) for m in self.markers], np.float64)
        self.marker_length = [0] * len(self.species)
        for _, r in rows:
            self.marker_length[index[r['species_id']]] += int(r['gene_length'])


def stream_reads(paths, out, read_length=None, max_reads=None):
    """The reads of the FASTA / FASTQ files as `>id_length` records on `out` -> (reads, bases).  The id is the header up to
    its first blank; with read_length shorter reads are dropped and longer ones cut; max_reads ends the stream."""
    reads = bases = 0

    def emit(name, seq):
        nonlocal reads, bases
        if read_length:
            if len(seq) < read_length:
                return False
            seq = seq[:read_length]
        out.write('>%s_%d\n%s\n' % (name, len(seq), seq))
        reads += 1
        bases += len(seq)
        return reads == max_reads

    for path in paths:
        with utility.iopen(path) as handle:
            name, parts, pending = None, [], None
            while True:
                line = pending if pending is not None else handle.readline()
                pending = None
                if not line:
                    break
                if name is None:
                    if line[0] in '>@':
                        name, parts = line[1:].rstrip('\n').split(' ')[0].split()[0], []
                    continue
                if line[0] == '+':                              # FASTQ: as many quality characters as bases follow
                    seq = ''.join(parts)
                    have = 0
                    while have < len(seq):
                        q = handle.readline()
                        if not q:
                            break
                        have += len(q) - 1
                    if emit(name, seq):
                        return reads, bases
                    name = None
                elif line[0] in '>@':                           # the next record: this one was FASTA
                    if emit(name, ''.join(parts)):
                        return reads, bases
                    name, pending = None, line
                else:
                    parts.append(line.rstrip('\n'))
            if name is not None and emit(name, ''.join(parts)):
                return reads, bases
    return reads, bases


def map_reads(args):
    """stream | hs-blastn align -outfmt 6 -> species/temp/alignments.m8; reads<TAB>bp -> species/temp/read_count.txt."""
    temp = os.path.join(args['outdir'], 'species', 'temp')
    command = [args['hs-blastn'], 'align', '-word_size', str(args['word_size']), '-query', '/dev/stdin',
               '-db', os.path.join(args['db'], 'marker_genes', 'phyeco.fa'), '-outfmt', '6', '-num_threads', str(args['threads']),
               '-out', os.path.join(temp, 'alignments.m8'), '-evalue', '1e-3']
    args['log'].write('command: <reads as >id_length FASTA> | %s\n' % ' '.join(command))
    process = subprocess.Popen(command, stdin=subprocess.PIPE, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    try:
        counts = stream_reads([p for p in (args['m1'], args['m2']) if p], process.stdin, args['read_length'], args['max_reads'])
        process.stdin.close()
    except BrokenPipeError:
        counts = None
    err = process.stderr.read()
    process.stdout.close()
    if process.wait() != 0 or counts is None:
        sys.exit("\nError encountered executing:\n%s\n\nError message:\n%s\n" % (' '.join(command), err))
    with open(os.path.join(temp, 'read_count.txt'), 'w') as handle:
        handle.write('%s\t%s' % counts)


def classify(ctx, text, mdb, aln_cov, chunk_bytes=0, hash_bits=0, py_state=None, np_state=None):
    """-> (per-species reads, per-species aln sums, the device step's dict)."""
    from midas_amd import abi
    hits = ctx.species_classify(text, mdb.gene_names, mdb.gene_species, mdb.gene_marker, len(mdb.species), mdb.cutoff, aln_cov,
                                chunk_bytes=chunk_bytes, hash_bits=hash_bits)
    t0 = time()
    reads, bases, _ = abi.species_assign(hits['indptr'], hits['hit_species'], hits['hit_aln'], hits['uniq_reads'], hits['uniq_aln'],
                                         py_state=py_state, np_state=np_state)
    hits['chain_ms'] = (time() - t0) * 1e3
    return reads, bases, hits


def abundance(mdb, reads, bases):
    """-> ([(species_id, count, coverage, relative abundance)] sorted by count, total coverage)."""
    cov = [float(int(b)) / length if n > 0 else 0.0 for n, b, length in zip(reads, bases, mdb.marker_length)]
    total = sum(cov)
    order = sorted(range(len(mdb.species)), key=lambda k: int(reads[k]), reverse=True)
    return [(mdb.species[k], int(reads[k]), cov[k], cov[k] / total if total > 0 else 0) for k in order], total


def write_abundance(outdir, rows):
    with open(os.path.join(outdir, 'species', 'species_profile.txt'), 'w') as handle:
        handle.write('\t'.join(['species_id', 'count_reads', 'coverage', 'relative_abundance']) + '\n')
        for row in rows:
            handle.write('\t'.join(str(x) for x in row) + '\n')


def run_pipeline(args):
    from midas_amd import abi
    mdb = MarkerDatabase(args['db'], args['mapid'])
    m8 = os.path.join(args['outdir'], 'species', 'temp', 'alignments.m8')
    if not args['classify']:
        start = time()
        print("\nAligning reads to marker-genes database")
        args['log'].write("\nAligning reads to marker-genes database\n")
        map_reads(args)
        print("  %s minutes" % round((time() - start) / 60, 2))
        print("  %s Gb maximum memory" % utility.max_mem_usage())

    start = time()
    print("\nClassifying reads")
    args['log'].write("\nClassifying reads\n")
    if args.get('seed') is not None:
        import random
        random.seed(args['seed'])
        np.random.seed(args['seed'])
    text = np.fromfile(m8, np.uint8)
    with abi.Context(0) as ctx:         # raises if the HIP library or the GPU is missing: no fallback
        try:
            reads, bases, hits = classify(ctx, text, mdb, args['aln_cov'])
        except abi.MidasSnpsError as e:
            sys.exit("\nError: %s: %s\n" % (m8, e))
    print("  total alignments: %s" % hits['lines'])
    print("  uniquely mapped reads: %s" % hits['unique'])
    print("  ambiguously mapped reads: %s" % hits['ambiguous'])
    print("  %s minutes" % round((time() - start) / 60, 2))
    print("  %s Gb maximum memory" % utility.max_mem_usage())

    start = time()
    print("\nEstimating species abundance")
    args['log'].write("\nEstimating species abundance\n")
    rows, total = abundance(mdb, reads, bases)
    print("  total marker-gene coverage: %s" % round(total, 3))
    print("  %s minutes" % round((time() - start) / 60, 2))
    print("  %s Gb maximum memory" % utility.max_mem_usage())
    write_abundance(args['outdir'], rows)
    if args['remove_temp']:
        shutil.rmtree(os.path.join(args['outdir'], 'species', 'temp'))
