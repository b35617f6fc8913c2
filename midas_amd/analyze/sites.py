"""What snp_diversity.py and call_consensus.py share on the host: the species directory (abi.SitesTables), the sample
selection of fetch_samples (midas/analyze/parse_snps.py:166-210) and the per-site mask of everything the info
table and the options decide by themselves.  Whatever depends on a frequency or a depth is the device's (Context.sites_scan)."""
import os
import sys

import numpy as np

from midas_amd import abi


class Sample:
    def __init__(self, id, index, mean_depth, fract_cov):
        self.id, self.index, self.mean_depth, self.fract_cov = id, index, mean_depth, fract_cov


def open_tables(indir):
    try:
        return abi.SitesTables(indir.rstrip('/') or indir)
    except abi.MidasSnpsError as e:
        sys.exit("\nError: %s\n" % e.message)


def fetch_samples(tables, mean_depth=0, fract_cov=0, max_samples=float('inf'), keep_samples=None, exclude_samples=None,
                  rand_samples=None, zero_depth_ok=False):
    """parse_snps.fetch_samples: the rows of snps_summary.txt that pass, in file order; a sample's matrix column is its row.
    keep_samples / exclude_samples are the option strings as given, and `in` is the reference's test on them.
    --rand_samples: the reference's two lines for it cannot run under Python 3; their intent is
    np.random.choice(list of ids, n, replace=False), and the kept samples stay in file order.
    zero_depth_ok: the caller never divides by a sample's mean_coverage (strain_tracking.py), so 0 is no error."""
    ids = tables.strings('sample_id')
    samples = {}
    for index, id in enumerate(ids):
        cov, fr = float(tables.mean_coverage[index]), float(tables.fraction_covered[index])
        if fr < fract_cov or cov < mean_depth:
            continue
        if keep_samples and id not in keep_samples:
            continue
        if exclude_samples and id in exclude_samples:
            continue
        if len(samples) >= max_samples:
            continue
        if id in samples:
            sys.exit("\nError: %s/snps_summary.txt lists the sample %s twice\n" % (tables.dir, id))
        samples[id] = Sample(id, index, cov, fr)
    if len(samples) == 0:
        sys.exit("\nError: no samples satisfied your selection criteria.\nTry running again with more lenient parameters\n")
    if rand_samples:
        if rand_samples > len(samples):
            sys.exit("\nError: --rand_samples cannot exceed the number of samples\n")
        chosen = set(np.random.choice(list(samples.keys()), rand_samples, replace=False).tolist())
        samples = {k: v for k, v in samples.items() if k in chosen}
    for s in samples.values():
        if s.index >= tables.n_columns or s.index >= tables.freq_columns:
            sys.exit("\nError: %s: sample %s is row %d of snps_summary.txt, but the matrices have %d sample columns\n"
                     % (tables.dir, s.id, s.index + 1, min(tables.n_columns, tables.freq_columns)))
        if s.mean_depth == 0 and not zero_depth_ok:         # (depth / mean_depth at the first site: ZeroDivisionError in the reference)
            sys.exit("\nError: %s/snps_summary.txt: sample %s has mean_coverage 0\n" % (tables.dir, s.id))
    return samples


def info_mask(tables, locus_type=None, site_type=None):
    """GenomicSite.filter's tests on the info table alone: ref_allele in ACGT, --locus_type, --site_type."""
    first, length = tables.first_bytes('ref_allele')
    mask = (length == 1) & np.isin(first, np.frombuffer(b'ATCG', np.uint8))
    if locus_type:
        mask &= tables.equals('locus_type', locus_type)
    if site_type:
        mask &= tables.equals('site_type', site_type)
    return mask


def read_site_list(path):
    with open(path) as f:
        return [line.rstrip() for line in f]


def scan(ctx, tables, samples, mask, n_sites, args, flags, classes=None, **kw):
    """Context.sites_scan over the first n_sites rows for the selected samples; a malformed row ends the command with the
    file and the line (the reference dies in float() / int() there).  classes = (site_class [n], n_classes):
    Context.sites_scan_classes, the sums once per class."""
    order = list(samples.values())
    call, lead = ctx.sites_scan, ()
    if classes is not None:
        call, lead = ctx.sites_scan_classes, (np.ascontiguousarray(classes[0][:n_sites], np.uint8), int(classes[1]))
    try:
        return call(tables.freq_text, tables.depth_text, np.ascontiguousarray(mask[:n_sites], np.uint8), *lead,
                    [s.index for s in order], [s.mean_depth for s in order], int(args['site_depth']), float(args['site_ratio']),
                    float(args['allele_support']), float(args['site_prev']), float(args['site_maf']),
                    max_sites=-1 if args['max_sites'] == float('inf') else int(args['max_sites']), flags=flags,
                    group_rows=int(args.get('group_rows', 0) or 0), chunk_bytes=int(args.get('chunk_bytes', 0) or 0), **kw)
    except abi.MidasSnpsError as e:
        exit_bad_row(tables, order, e)


def exit_bad_row(tables, order, e):
    """End the command on a device call's error: a malformed row with its file and line, anything else as it is."""
    bad = getattr(e, 'bad', None)
    if not bad:
        sys.exit("\nError: %s\n" % e.message)
    name = 'snps_freq.txt' if bad[0] in (1, 3) else 'snps_depth.txt'
    if bad[0] == 3:         # (round() of nan or inf: ValueError / OverflowError in the reference)
        what = "sample %s: the frequency is not a finite number, so --consensus cannot round it" % order[bad[2]].id
    elif bad[0] == 6:       # (maf / depth: ZeroDivisionError in the reference)
        what = "the depths of the samples kept at the site sum to 0, so --weight_by_depth has no frequency for it"
    else:
        what = "the row has fewer sample columns than the samples in use" if bad[2] < 0 else \
            "sample %s: the cell is not %s" % (order[bad[2]].id, 'a number' if bad[0] == 1 else 'an integer')
    sys.exit("\nError: %s, line %d: %s\n" % (os.path.join(tables.dir, name), bad[1] + 2, what))


def device_context():
    return abi.Context(int(os.environ.get("LOCAL_RANK", "0")))
