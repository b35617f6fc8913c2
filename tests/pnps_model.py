"""A sequential model of Context.sites_scan_classes (midas_sites_scan_classes), built from the model of sites_scan alone
(tests/analyze_model.py): class c is sites_scan with the mask site_mask & (site_class == c).  Under max_sites N the retained
sites of all classes count together, so the union mask is run first, without a cap and with its keep flags dumped; the rows
behind the N-th kept site are then switched off in every class's mask.  n_kept, no_gene and the other statistics are the union
run's (with the cap)."""
import json
import os

import numpy as np

from midas_amd import abi
from tests import analyze_model as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pnps_vectors.json")


def load_vectors():
    with open(GOLDEN) as f:
        return json.load(f)


def sites_scan_classes(freq_text, depth_text, site_mask, site_class, n_classes, sample_col, mean_depth, site_depth, site_ratio,
                       allele_support, site_prev, site_maf, **kw):
    mask = np.asarray(site_mask, np.uint8)
    N = int(mask.shape[0])
    cls = np.zeros(N, np.uint8) if site_class is None else np.asarray(site_class, np.uint8)
    flags = kw.get('flags', 0)
    if not 1 <= n_classes <= abi.SITES_MAX_CLASSES or (site_class is None and n_classes > 1) or flags & abi.SITES_SEQ or np.any((mask != 0) & (cls >= n_classes)):
        raise abi.MidasSnpsError(abi.ERR_INVALID_ARG, "invalid argument")
    args = (sample_col, mean_depth, site_depth, site_ratio, allele_support, site_prev, site_maf)
    union = M.sites_scan(freq_text, depth_text, mask, *args, **kw)
    max_sites = kw.get('max_sites', -1)
    live = np.ones(N, bool)
    if max_sites >= 0:
        free = dict(kw, max_sites=-1, dump=True)
        free.pop('dump_keep', None)
        kept_rows = np.flatnonzero(M.sites_scan(freq_text, depth_text, mask, *args, **free)['keep'])
        live[:] = False
        if max_sites > 0:
            live[:(int(kept_rows[max_sites - 1]) + 1) if len(kept_rows) >= max_sites else N] = True
    out = dict(union)
    if flags & abi.SITES_SUMS:
        per = dict(kw, max_sites=-1, dump=False, dump_keep=False)
        blocks = [M.sites_scan(freq_text, depth_text, mask & live & (cls == c), *args, **per) for c in range(n_classes)]
        for k in ('pi', 'snps', 'sites', 'depth'):
            out[k] = np.stack([b[k] for b in blocks])
    return out


class ModelContext(M.ModelContext):
    """Stands in for abi.Context in pnps.run_pipeline."""

    def sites_scan_classes(self, *a, **kw):
        return sites_scan_classes(*a, **kw)
