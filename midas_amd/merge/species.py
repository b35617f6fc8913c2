"""merge_species.py: the samples' species/species_profile.txt -> relative_abundance.txt, coverage.txt, count_reads.txt and
species_prevalence.txt (midas/merge/species.py).  The profiles are read by the library's host threads, parsed on the device into
three [species][sample] matrices, and the per-species means, medians, prevalence and order are formed there too
(csrc/species_merge.hip); this module lists the samples by the reference's rules and names the files.

Stricter than the reference, each an error naming the file, the line and the species or column (the earliest such line in the
order of samples, then lines): a species id that species_info.txt does not have (the reference raises KeyError), a species of
species_info.txt without a line in a profile (the reference writes a shorter, misaligned row), a species on two lines of one
profile, a header without one of species_id / count_reads / coverage / relative_abundance, a cell that float() / int() does not
take, a coverage or relative abundance that is not finite, a count_reads beyond 64 bits.
"""

import os
import sys
from time import time

README = """Output of merge_species.py (serves what `merge_midas.py species` serves)

count_reads.txt         reads mapped to the 15 marker genes, a row a species, a column a sample
coverage.txt            mean read depth over the 15 marker genes (bases of mapped reads / bases of the marker genes)
relative_abundance.txt  the values of coverage.txt scaled to sum to 1.0 over the species of a sample
                        the three are tab-separated matrices: the header names the samples, the first field of a row the species,
                        rows in the order of species_info.txt
species_prevalence.txt  a row a species, most prevalent first:
                        mean_coverage, median_coverage      mean and median of the species' coverage over the samples
                        mean_abundance, median_abundance    the same of its relative abundance
                        prevalence                          samples in which its coverage is at least %s

More on every species: %s/species_info.txt
"""


class Sample:
    def __init__(self, dir):
        self.dir = dir
        self.id = os.path.basename(dir)
        self.path = '%s/species/species_profile.txt' % dir


def identify_samples(args):
    """midas/merge/species.py:17-26, 90-104: warnings and their texts are the reference's."""
    samples = []
    for d in args['indirs']:
        sample = Sample(d)
        if not os.path.exists(sample.path):
            sys.stderr.write("Warning: missing/incomplete output: %s\n" % d)
        elif sample.id in [s.id for s in samples]:
            sys.stderr.write("Warning: sample_id '%s' specified more than one time.\nSkipping: %s\n" % (sample.id, sample.dir))
        else:
            samples.append(sample)
    if len(samples) == 0:
        sys.exit("\nError: no samples with species profiles\n")
    if args['max_samples'] is not None and len(samples) > args['max_samples']:
        samples = samples[0:args['max_samples']]
    return samples


def read_species_ids(db):
    """The species ids of <db>/species_info.txt in row order, each once (utility.parse_file: a line whose field count is not
    the header's is dropped; read_annotations keys a dict by species_id)."""
    path = os.path.join(db, 'species_info.txt')
    if not os.path.isfile(path):
        sys.exit("\nError: Could not locate species info: %s\n" % path)
    ids = {}
    with open(path) as handle:
        fields = handle.readline().rstrip('\n').split('\t')
        if 'species_id' not in fields:
            sys.exit("\nError: %s has no species_id column\n" % path)
        col = len(fields) - 1 - fields[::-1].index('species_id')
        for line in handle:
            values = line.rstrip('\n').split('\t')
            if len(values) == len(fields):
                ids[values[col]] = None
    if not ids:
        sys.exit("\nError: %s lists no species\n" % path)
    return list(ids)


def merge(ctx, samples, species_ids, sample_depth, chunk_bytes=0, lds_bound=0, threads=0):
    """-> abi.SpeciesMerge of the samples' profiles (the device step)."""
    return ctx.species_merge([s.path for s in samples], species_ids, sample_depth, chunk_bytes=chunk_bytes, lds_bound=lds_bound, threads=threads)


def write_readme(args):
    with open('%s/readme.txt' % args['outdir'], 'w') as handle:
        handle.write(README % (args['sample_depth'], args['db']))


def run_pipeline(args):
    from midas_amd import abi
    trace = args.get('profile') or os.environ.get('MIDAS_SNPS_TRACE')
    samples = identify_samples(args)
    species_ids = read_species_ids(args['db'])
    print("Merging the species profiles of %d samples over %d species" % (len(samples), len(species_ids)))
    start = time()
    with abi.Context(0) as ctx:         # raises if the HIP library or the GPU is missing: no fallback
        try:
            res = merge(ctx, samples, species_ids, args['sample_depth'], chunk_bytes=int(args.get('chunk_bytes') or 0))
        except abi.MidasSnpsError as e:
            sys.exit("\nError: %s\n" % e.message)
        with res:
            merged = time()
            res.write(args['outdir'], [s.id for s in samples])
            wrote = time()
            if trace:
                print("  %d lines of %d bytes in %d groups, %d cells through the host's parser" % (res.lines, res.text_bytes, res.groups, res.side_cells))
                for name, ms in zip(abi.SPECIES_MERGE_PHASES, res.ms):
                    print("  %-18s %10.3f ms" % (name, ms))
                print("  %-18s %10.3f ms" % ('write', (wrote - merged) * 1e3))
    write_readme(args)
    print("  %s minutes" % round((time() - start) / 60, 2))
