"""MI355X-native strain_tracking.py: the host side.

Mirrors midas/analyze/track_strains.py.  id_markers: count_alleles and the marker decision for every site are one device
call that brings down the marker rows alone; the table is written natively.  track_markers: the marker file is walked against
snps_info.txt with one cursor here (as --site_list is in diversity.site_mask), which leaves one byte per site -- no marker, the
major or the minor allele; the device calls every (matched site, sample) into a bit matrix and counts the shared bits of every
pair of samples; the pair table is written natively.  Nothing here depends on a frequency or a depth.
"""
import os
import sys

import numpy as np

from midas_amd import abi
from midas_amd.analyze import sites as S

INF = float('inf')


def rows_in_use(n_sites, max_sites):
    """-> (rows called, rows read): `if index >= max_sites: break` sits behind the read of row `index`."""
    n_call = n_sites if max_sites == INF else max(0, min(n_sites, int(max_sites)))
    return n_call, min(n_sites, n_call + 1)


def allele_codes(tables, name, n):
    """Per site: the allele's index into abi.ALLELE_LETTERS, 255 for any other string."""
    first, length = tables.first_bytes(name)
    lut = np.full(256, 255, np.uint8)
    for k, c in enumerate(abi.ALLELE_LETTERS):
        lut[ord(c)] = k
    return np.where(length[:n] == 1, lut[first[:n]], 255).astype(np.uint8)


def _exit_bad(tables, order, e):
    """A site the reference cannot call either (KeyError on the letter, round() of a non-finite product), or a malformed row."""
    bad = getattr(e, 'bad', None)
    if not bad or bad[0] < 3:
        S.exit_bad_row(tables, order, e)
    kind, row, slot = bad
    if kind == 3:
        sys.exit("\nError: %s, line %d: sample %s: frequency x depth is not a finite number\n"
                 % (os.path.join(tables.dir, 'snps_freq.txt'), row + 2, order[slot].id))
    name = 'minor_allele' if kind == 4 else 'major_allele'
    sys.exit("\nError: %s, line %d: sample %s has the %s '%s', which is none of A, T, C, G\n"
             % (os.path.join(tables.dir, 'snps_info.txt'), row + 2, order[slot].id, name, tables.strings(name)[row]))


def _device_options(args):
    return dict(group_rows=int(args.get('group_rows', 0) or 0), chunk_bytes=int(args.get('chunk_bytes', 0) or 0))


def _write(fn, *a):
    try:
        fn(*a)
    except abi.MidasSnpsError as e:
        sys.exit("\nError: %s\n" % e.message)


def id_markers(args, make_context=S.device_context):
    """track_strains.id_markers.  make_context: tests substitute a CPU double of the device."""
    tables = S.open_tables(args['indir'])
    samples = S.fetch_samples(tables, keep_samples=args['samples'], zero_depth_ok=True)
    order = list(samples.values())
    n_call, n_parse = rows_in_use(tables.n_sites, args['max_sites'])
    ctx = make_context()
    try:
        res = ctx.sites_id_markers(tables.freq_text, tables.depth_text, allele_codes(tables, 'minor_allele', n_call),
                                   allele_codes(tables, 'major_allele', n_call), [s.index for s in order], float(args['min_freq']),
                                   int(args['min_reads']), int(args['allele_prev']), n_parse=n_parse, **_device_options(args))
    except abi.MidasSnpsError as e:
        _exit_bad(tables, order, e)
    finally:
        ctx.close()
    _write(tables.write_markers, args['out'], res['rows'])
    print("\n%s total disriminative alleles found" % len(res['rows']))
    return res


def read_markers(path):
    """utility.parse_file over the marker list: tab-separated with a header, a row of another width is skipped."""
    with open(path) as f:
        header = next(f, None)
        if header is None:
            return []
        fields = header.rstrip('\n').split('\t')
        rows = [dict(zip(fields, v)) for v in (line.rstrip('\n').split('\t') for line in f) if len(v) == len(fields)]
    if rows and ('site_id' not in rows[0] or 'allele' not in rows[0]):
        sys.exit("\nError: %s: the header lacks the column site_id or allele\n" % path)
    return rows


def marker_sites(tables, markers, max_sites):
    """call_markers' walk over snps_info.txt with one cursor into the marker list -> (which uint8 [rows called]: 0 no marker,
    1 the marker is the site's major, 2 its minor allele; rows read).  A listed site that is absent or out of order blocks all
    after it; the loop ends with the list; a marker allele that is neither of the site's two is used up without a call."""
    n_call, n_parse = rows_in_use(tables.n_sites, max_sites)
    ids, major, minor = tables.strings('site_id'), tables.strings('major_allele'), tables.strings('minor_allele')
    which = np.zeros(n_call, np.uint8)
    cursor, seen = 0, set()
    for i in range(n_call):
        if ids[i] != markers[cursor]['site_id']:
            continue
        if ids[i] in seen:
            sys.exit("\nError: %s/snps_info.txt, line %d: the site %s is listed twice\n" % (tables.dir, i + 2, ids[i]))
        seen.add(ids[i])
        allele = markers[cursor]['allele']
        which[i] = 1 if allele == major[i] else 2 if allele == minor[i] else 0
        cursor += 1
        if cursor == len(markers):
            return which[:i + 1], i + 1
    return which, n_parse


def track_markers(args, make_context=S.device_context):
    """track_strains.track_markers: every sample of snps_summary.txt (--max_samples is accepted and never applied)."""
    tables = S.open_tables(args['indir'])
    samples = S.fetch_samples(tables, zero_depth_ok=True)
    order = list(samples.values())
    print("Determining marker alleles present in each sample")
    markers = read_markers(args['markers'])
    if not markers:
        sys.exit("\nError: no marker alleles found in file: %s\n" % args['markers'])
    which, n_parse = marker_sites(tables, markers, args['max_sites'])
    ctx = make_context()
    try:
        res = ctx.sites_track_markers(tables.freq_text, tables.depth_text, which, [s.index for s in order], float(args['min_freq']),
                                      int(args['min_reads']), n_parse=n_parse, **_device_options(args))
    except abi.MidasSnpsError as e:
        _exit_bad(tables, order, e)
    finally:
        ctx.close()
    print("Quantifying sharing of marker alleles between samples")
    for index in range(0, len(order) * (len(order) - 1) // 2, 500):
        print("%s sample pairs processed" % index)
    _write(tables.write_pairs, args['out'], [s.index for s in order], res['both'])
    return res
