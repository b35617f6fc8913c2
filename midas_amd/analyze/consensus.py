"""MI355X-native call_consensus.py: the host side.

Mirrors scripts/call_consensus.py: the site loop (:183-213) is one device call that returns, per sample, the
consensus bytes of the retained sites as one contiguous run; write_consensus (:160-168) is unchanged in what it prints.  As in
the reference, --keep_samples and --exclude_samples are accepted and printed but never reach the sample selection, and a
--site_list is a set that REPLACES the site filters (prevalence, frequency, locus and site type, reference allele).
"""
import sys

import numpy as np

from midas_amd import abi
from midas_amd.analyze import sites as S


def compute(args, tables, samples, ctx):
    flags = abi.SITES_SEQ
    if args['site_list']:
        listed = set(S.read_site_list(args['site_list']))
        mask = np.fromiter((i in listed for i in tables.strings('site_id')), bool, tables.n_sites)
        flags |= abi.SITES_MASK_ONLY
    else:
        mask = S.info_mask(tables, args['locus_type'], args['site_type'])
    minor, n_minor = tables.first_bytes('minor_allele')
    major, n_major = tables.first_bytes('major_allele')
    # an allele that is not one letter ('NA' at a site no sample covers) travels as a placeholder byte; it reaches the output
    # only if some sample is kept there with depth > 0, and then the sequences are put together on the host
    minor = np.where(n_minor == 1, minor, 1).astype(np.uint8)
    major = np.where(n_major == 1, major, 2).astype(np.uint8)
    res = S.scan(ctx, tables, samples, mask, tables.n_sites, args, flags, minor=minor, major=major, dump_keep=True)
    seq = res['seq']
    res['seq'] = [row.tobytes() for row in seq]
    if seq.size and int(seq.min()) <= 2:
        kept = np.flatnonzero(res['keep'])
        names = {1: tables.strings('minor_allele'), 2: tables.strings('major_allele')}
        res['seq'] = [b''.join(names[b][kept[k]].encode() if b <= 2 else bytes([b]) for k, b in enumerate(row.tolist())) for row in seq]
    return res


def percent_missing(row):
    return round(100 * row.count(b'-') / float(len(row)), 2) if len(row) > 0 else 'NA'


def write_consensus(args, samples, seq):
    order = {s.id: k for k, s in enumerate(samples.values())}
    with open(args['out'], 'w') as out:
        for sample_id in sorted(samples):
            sample, row = samples[sample_id], seq[order[sample_id]]
            desc = [('length', len(row)), ('percent_missing', percent_missing(row)), ('mean_depth', round(sample.mean_depth, 2))]
            out.write('>' + sample.id + '\t' + ' '.join('%s=%s' % kv for kv in desc) + '\n')
            out.write(row.decode('latin-1') + '\n')


def run_pipeline(args, make_context=S.device_context):
    """scripts/call_consensus.py:171-216.  make_context: tests substitute a CPU double of the device."""
    tables = S.open_tables(args['indir'])
    samples = S.fetch_samples(tables, args['sample_depth'], args['fract_cov'], args['max_samples'])
    ctx = make_context()
    try:
        res = compute(args, tables, samples, ctx)
    finally:
        ctx.close()
    write_consensus(args, samples, res['seq'])
    return res
