"""A seeded species directory in the shape `merge_midas.py snps` writes (snps_summary.txt, snps_info.txt, snps_freq.txt,
snps_depth.txt), for tests and measurements.  The freq cells are '{:.3g}' of k / 1000, as the merge formats them; the matrices
are assembled as bytes with numpy, so a 2 M x 50 table takes seconds rather than minutes."""
import os

import numpy as np

FREQ_PALETTE = ['{:.3g}'.format(k / 1000.0) for k in range(1001)] + ['1e-05', '0.0123', '2.5e-05']


def _matrix_bytes(first_site, idx, palette):
    """Rows '<site id>\\t<cell>\\t...\\n' for idx [rows, cols] into palette (list of str)."""
    rows, cols = idx.shape
    width = max(len(p) for p in palette)
    chars = np.zeros((len(palette), width), np.uint8)
    plen = np.zeros(len(palette), np.int64)
    for k, p in enumerate(palette):
        b = p.encode()
        chars[k, :len(b)] = np.frombuffer(b, np.uint8)
        plen[k] = len(b)
    ids = [str(first_site + r + 1).encode() for r in range(rows)]
    id_len = np.array([len(b) for b in ids], np.int64)
    clen = plen[idx] + 1                               # the cell and the tab before it
    row_len = id_len + clen.sum(axis=1) + 1
    row_off = np.concatenate([[0], np.cumsum(row_len)])
    out = np.full(int(row_off[-1]), ord('\t'), np.uint8)
    out[row_off[1:] - 1] = ord('\n')
    id_pool = np.frombuffer(b''.join(ids), np.uint8)
    id_off = np.concatenate([[0], np.cumsum(id_len)])[:-1]
    pos = np.repeat(row_off[:-1] - id_off, id_len) + np.arange(id_pool.shape[0])
    out[pos] = id_pool
    cell_off = row_off[:-1, None] + id_len[:, None] + np.cumsum(clen, axis=1) - clen + 1
    flat_idx, flat_off = idx.ravel(), cell_off.ravel()
    for j in range(width):
        m = plen[flat_idx] > j
        out[flat_off[m] + j] = chars[flat_idx[m], j]
    return out


def write_species_dir(path, n_sites, n_samples, seed=0, n_genes=0, block=100000, max_depth=60):
    """-> dict(sample_ids).  Sites are CDS / 1D..4D with genes in runs when n_genes > 0, else IGR."""
    os.makedirs(path, exist_ok=True)
    rng = np.random.default_rng(seed)
    sample_ids = ['sample_%03d' % k for k in range(n_samples)]
    mean = rng.uniform(4.0, 30.0, n_samples)
    with open(os.path.join(path, 'snps_summary.txt'), 'w') as f:
        f.write('\t'.join(['sample_id', 'genome_length', 'covered_bases', 'fraction_covered', 'mean_coverage']) + '\n')
        for k in range(n_samples):
            f.write('%s\t%d\t%d\t%s\t%s\n' % (sample_ids[k], n_sites, n_sites // 2, repr(float(rng.uniform(0.4, 1.0))), repr(float(mean[k]))))
    header = ('\t'.join(['site_id'] + sample_ids) + '\n').encode()
    depth_palette = [str(k) for k in range(max_depth + 1)]
    with open(os.path.join(path, 'snps_freq.txt'), 'wb') as ff, open(os.path.join(path, 'snps_depth.txt'), 'wb') as fd, \
            open(os.path.join(path, 'snps_info.txt'), 'w') as fi:
        ff.write(header)
        fd.write(header)
        fi.write('\t'.join(['site_id', 'ref_id', 'ref_pos', 'ref_allele', 'major_allele', 'minor_allele', 'count_samples', 'count_a',
                            'count_c', 'count_g', 'count_t', 'locus_type', 'gene_id', 'snp_type', 'site_type', 'amino_acids']) + '\n')
        per_gene = max(1, n_sites // n_genes) if n_genes else 0
        for r0 in range(0, n_sites, block):
            rows = min(block, n_sites - r0)
            variable = rng.random((rows, 1)) < 0.3
            fi_idx = np.where(variable & (rng.random((rows, n_samples)) < 0.5), rng.integers(0, len(FREQ_PALETTE), (rows, n_samples)),
                              np.where(rng.random((rows, n_samples)) < 0.05, 1000, 0))
            di = np.minimum(rng.poisson(mean[None, :] * rng.uniform(0.3, 1.6, (rows, 1))), max_depth)
            ff.write(_matrix_bytes(r0, fi_idx, FREQ_PALETTE).tobytes())
            fd.write(_matrix_bytes(r0, di, depth_palette).tobytes())
            al = rng.integers(0, 4, (rows, 3))
            st = rng.integers(1, 5, rows)
            lines = []
            for r in range(rows):
                site = r0 + r
                a, b, c = 'ACGT'[al[r, 0]], 'ACGT'[al[r, 1]], 'ACGT'[(al[r, 1] + 1 + al[r, 2] % 3) % 4]
                if n_genes:
                    lines.append('%d\tcontig_1\t%d\t%s\t%s\t%s\t%d\t0\t0\t0\t0\tCDS\tgene_%05d\tbi\t%dD\t\n'
                                 % (site + 1, site + 1, a, b, c, n_samples, min(site // per_gene, n_genes - 1), st[r]))
                else:
                    lines.append('%d\tcontig_1\t%d\t%s\t%s\t%s\t%d\t0\t0\t0\t0\tIGR\t\tbi\t\t\n' % (site + 1, site + 1, a, b, c, n_samples))
            fi.write(''.join(lines))
    return dict(sample_ids=sample_ids)


PRIVATE_FREQ = [1000, 1000, 1000, 800, 500, 333, 250, 120, 100, 1001]      # indices into FREQ_PALETTE: 1, 0.8, ..., 0.1, 1e-05


def write_strain_species_dir(path, n_sites, n_samples, seed=0, block=100000, max_depth=60, private=0.2, shared=0.06, common=0.03):
    """-> dict(sample_ids).  A species for strain_tracking.py: every site is fixed (freq 0 in all samples) unless it is planted --
    with probability `private` one sample carries the minor allele, with probability `shared` two to four samples do, with
    probability `common` about half of them do -- at a frequency out of PRIVATE_FREQ.  About 3 % of the depths are 0."""
    os.makedirs(path, exist_ok=True)
    rng = np.random.default_rng(seed)
    sample_ids = ['sample_%03d' % k for k in range(n_samples)]
    mean = rng.uniform(6.0, 30.0, n_samples)
    with open(os.path.join(path, 'snps_summary.txt'), 'w') as f:
        f.write('\t'.join(['sample_id', 'genome_length', 'covered_bases', 'fraction_covered', 'mean_coverage']) + '\n')
        for k in range(n_samples):
            f.write('%s\t%d\t%d\t%s\t%s\n' % (sample_ids[k], n_sites, n_sites // 2, repr(float(rng.uniform(0.4, 1.0))), repr(float(mean[k]))))
    header = ('\t'.join(['site_id'] + sample_ids) + '\n').encode()
    depth_palette = [str(k) for k in range(max_depth + 1)]
    planted = np.array(PRIVATE_FREQ)
    with open(os.path.join(path, 'snps_freq.txt'), 'wb') as ff, open(os.path.join(path, 'snps_depth.txt'), 'wb') as fd, \
            open(os.path.join(path, 'snps_info.txt'), 'w') as fi:
        ff.write(header)
        fd.write(header)
        fi.write('\t'.join(['site_id', 'ref_id', 'ref_pos', 'ref_allele', 'major_allele', 'minor_allele', 'count_samples', 'count_a',
                            'count_c', 'count_g', 'count_t', 'locus_type', 'gene_id', 'snp_type', 'site_type', 'amino_acids']) + '\n')
        for r0 in range(0, n_sites, block):
            rows = min(block, n_sites - r0)
            kind = rng.random(rows)
            carriers = np.where(kind < private, 1, np.where(kind < private + shared, rng.integers(2, 5, rows), 0))
            carried = ((kind >= private + shared) & (kind < private + shared + common))[:, None] & (rng.random((rows, n_samples)) < 0.5)
            for k in range(4):                             # a site's k-th carrier (two picks may fall on one sample)
                on = np.flatnonzero(carriers > k)
                carried[on, rng.integers(0, n_samples, on.shape[0])] = True
            fi_idx = np.where(carried, planted[rng.integers(0, len(planted), (rows, n_samples))], 0)
            di = np.minimum(rng.poisson(mean[None, :] * rng.uniform(0.3, 1.6, (rows, 1))), max_depth)
            di[rng.random((rows, n_samples)) < 0.03] = 0
            ff.write(_matrix_bytes(r0, fi_idx, FREQ_PALETTE).tobytes())
            fd.write(_matrix_bytes(r0, di, depth_palette).tobytes())
            al = rng.integers(0, 4, (rows, 3))
            fi.write(''.join('%d\tcontig_1\t%d\t%s\t%s\t%s\t%d\t0\t0\t0\t0\tIGR\t\tbi\t\t\n'
                             % (r0 + r + 1, r0 + r + 1, 'ACGT'[al[r, 0]], 'ACGT'[al[r, 1]], 'ACGT'[(al[r, 1] + 1 + al[r, 2] % 3) % 4], n_samples)
                             for r in range(rows)))
    return dict(sample_ids=sample_ids)


def write_genes_dir(path, n_genes, n_samples, seed=0, block=100000, palette_size=4093, absent=0.3):
    """-> dict(sample_ids).  One species directory in the shape `merge_midas.py genes` writes, for compare_genes.py:
    genes_copynum.txt holds repr() of doubles out of a seeded palette -- 17 significant digits in most, as the merge writes
    them, a share `absent` of the cells 0.0, a few scaled to e-07 / e+07; genes_presabs.txt and genes_depth.txt, which the
    command only wants to exist, hold their header line."""
    os.makedirs(path, exist_ok=True)
    rng = np.random.default_rng(seed)
    sample_ids = ['sample_%03d' % k for k in range(n_samples)]
    values = rng.gamma(2.0, 0.6, palette_size)
    values[rng.random(palette_size) < 0.1] *= 0.25                 # around the cutoffs
    scale = rng.random(palette_size)
    values = np.where(scale < 0.03, values * 1e-07, np.where(scale < 0.06, values * 1e+07, values))
    palette = ['0.0'] + [repr(float(v)) for v in values]
    header = ('\t'.join(['gene_id'] + sample_ids) + '\n').encode()
    for kind in ('presabs', 'depth'):
        with open(os.path.join(path, 'genes_%s.txt' % kind), 'wb') as f:
            f.write(header)
    with open(os.path.join(path, 'genes_copynum.txt'), 'wb') as f:
        f.write(header)
        for r0 in range(0, n_genes, block):
            rows = min(block, n_genes - r0)
            idx = np.where(rng.random((rows, n_samples)) < absent, 0, rng.integers(1, len(palette), (rows, n_samples)))
            f.write(_matrix_bytes(r0, idx, palette).tobytes())
    return dict(sample_ids=sample_ids)


def write_linked_genes_dir(path, n_genes, n_samples, seed=0, groups=None, block=10000, flip=0.01):
    """-> dict(sample_ids, group_of int32 [n_genes]: the planted group of every row, -1 none).  One species directory in the
    shape `merge_midas.py genes` writes, for gene_linkage.py.  Most genes are independent of one another at mixed prevalence
    (0.02 + 0.83 x a beta(0.6, 0.6) draw each: many rare, many common, none so near to core that chance alone links them).  groups: the sizes of the planted groups (default: one group for
    every 400 genes, 5 to 50 genes each); the members of a group stand at rows drawn without order and copy one presence
    profile with a share `flip` of their cells flipped, so the linked pairs are neither none nor a flood.  A present cell is a
    short decimal above 0.4, an absent one 0.0 or, one in ten, 0.21."""
    os.makedirs(path, exist_ok=True)
    rng = np.random.default_rng(seed)
    sample_ids = ['sample_%03d' % k for k in range(n_samples)]
    if groups is None:
        groups = [int(x) for x in rng.integers(5, 51, max(1, n_genes // 400))]
    groups = [int(x) for x in groups]
    if sum(groups) > n_genes:
        raise ValueError("the planted groups hold %d genes, the matrix %d" % (sum(groups), n_genes))
    group_of = np.full(n_genes, -1, np.int32)
    rows = rng.permutation(n_genes)[:sum(groups)]
    group_of[rows] = np.repeat(np.arange(len(groups), dtype=np.int32), groups)
    profiles = rng.random((len(groups), n_samples)) < rng.uniform(0.15, 0.85, (len(groups), 1))
    palette = ['0.0', '0.21'] + ['%.3f' % v for v in 0.4 + rng.gamma(2.0, 0.6, 62)]
    header = ('\t'.join(['gene_id'] + sample_ids) + '\n').encode()
    for kind in ('presabs', 'depth'):
        with open(os.path.join(path, 'genes_%s.txt' % kind), 'wb') as f:
            f.write(header)
    with open(os.path.join(path, 'genes_copynum.txt'), 'wb') as f:
        f.write(header)
        for r0 in range(0, n_genes, block):
            n = min(block, n_genes - r0)
            present = rng.random((n, n_samples)) < 0.02 + 0.83 * rng.beta(0.6, 0.6, (n, 1))
            g = group_of[r0:r0 + n]
            planted = g >= 0
            if planted.any():
                present[planted] = profiles[g[planted]] ^ (rng.random((int(planted.sum()), n_samples)) < flip)
            idx = np.where(present, rng.integers(2, len(palette), (n, n_samples)), (rng.random((n, n_samples)) < 0.1).astype(np.int64))
            f.write(_matrix_bytes(r0, idx, palette).tobytes())
    return dict(sample_ids=sample_ids, group_of=group_of)


def write_assoc_genes_dir(path, n_genes, n_samples, seed=0, associated=0.01, unnamed=0.05, block=10000):
    """-> dict(sample_ids, groups_path, planted bool [n_genes]).  One species directory in the shape `merge_midas.py genes`
    writes, for gene_assoc.py, with groups.txt beside the matrices: a share `unnamed` of the samples carries no label, the others
    are 'case' or 'control' at even odds.  Most genes are independent of the label at mixed prevalence (as in
    write_linked_genes_dir); a share `associated` of them is planted: present in 70 % of the cases and 25 % of the controls,
    with copy numbers half as high again in the cases.  A present cell is a short decimal above 0.4, an absent one 0.0 or, one
    in ten, 0.21: many tied zeros, as in the real matrices."""
    os.makedirs(path, exist_ok=True)
    rng = np.random.default_rng(seed)
    sample_ids = ['sample_%03d' % k for k in range(n_samples)]
    named = rng.random(n_samples) >= unnamed
    is_case = rng.random(n_samples) < 0.5
    named[:2], is_case[0], is_case[1] = True, True, False        # (both groups are never empty)
    groups_path = os.path.join(path, 'groups.txt')
    with open(groups_path, 'w') as f:
        f.write('sample_id\tlabel\n' + ''.join('%s\t%s\n' % (sample_ids[k], 'case' if is_case[k] else 'control') for k in range(n_samples) if named[k]))
    planted = rng.random(n_genes) < associated
    palette = ['0.0', '0.21'] + ['%.3f' % v for v in np.sort(0.4 + rng.gamma(2.0, 0.6, 62))]
    header = ('\t'.join(['gene_id'] + sample_ids) + '\n').encode()
    for kind in ('presabs', 'depth'):
        with open(os.path.join(path, 'genes_%s.txt' % kind), 'wb') as f:
            f.write(header)
    with open(os.path.join(path, 'genes_copynum.txt'), 'wb') as f:
        f.write(header)
        for r0 in range(0, n_genes, block):
            n = min(block, n_genes - r0)
            prevalence = 0.02 + 0.83 * rng.beta(0.6, 0.6, (n, 1))
            level = np.where(is_case, 0.70, 0.25)[None, :]
            p = np.where(planted[r0:r0 + n, None], level, prevalence)
            present = rng.random((n, n_samples)) < p
            value = rng.integers(2, 2 + 31, (n, n_samples))                                   # the lower half of the sorted palette
            value = np.where(planted[r0:r0 + n, None] & is_case[None, :], value + 31, value)    # the upper half for the cases of a planted gene
            idx = np.where(present, value, (rng.random((n, n_samples)) < 0.1).astype(np.int64))
            f.write(_matrix_bytes(r0, idx, palette).tobytes())
    return dict(sample_ids=sample_ids, groups_path=groups_path, planted=planted)


def write_pangenome_curve_dir(path, n_genes, n_samples, seed=0, block=10000):
    """-> dict(sample_ids, kind int8 [n_genes]).  One species directory in the shape `merge_midas.py genes` writes, for
    gene_curves.py: a core that erodes and a pangenome that keeps growing.  Every gene draws one of eight kinds: 0 present in
    every sample, 1 in all but one, 2 / 3 / 4 / 5 in about 97 %, 70 %, 30 % and 2 % of the samples, 6 in exactly one sample, 7
    in none (shares 15, 5, 10, 15, 20, 20, 10 and 5 %).  A present cell is a short decimal above 0.4, an absent one 0.0 or, one
    in ten, 0.21."""
    os.makedirs(path, exist_ok=True)
    rng = np.random.default_rng(seed)
    sample_ids = ['sample_%03d' % k for k in range(n_samples)]
    kind = rng.choice(8, n_genes, p=[0.15, 0.05, 0.10, 0.15, 0.20, 0.20, 0.10, 0.05]).astype(np.int8)
    level = np.array([1.0, 1.0, 0.97, 0.70, 0.30, 0.02, 0.0, 0.0])
    palette = ['0.0', '0.21'] + ['%.3f' % v for v in 0.4 + rng.gamma(2.0, 0.6, 62)]
    header = ('\t'.join(['gene_id'] + sample_ids) + '\n').encode()
    for name in ('presabs', 'depth'):
        with open(os.path.join(path, 'genes_%s.txt' % name), 'wb') as f:
            f.write(header)
    with open(os.path.join(path, 'genes_copynum.txt'), 'wb') as f:
        f.write(header)
        for r0 in range(0, n_genes, block):
            n = min(block, n_genes - r0)
            k = kind[r0:r0 + n]
            present = rng.random((n, n_samples)) < level[k][:, None]
            lone = rng.integers(0, n_samples, n)                       # the sample a gene of kind 1 misses, one of kind 6 has
            rows = np.arange(n)
            present[rows[k == 1], lone[k == 1]] = False
            present[rows[k == 6], lone[k == 6]] = True
            idx = np.where(present, rng.integers(2, len(palette), (n, n_samples)), (rng.random((n, n_samples)) < 0.1).astype(np.int64))
            f.write(_matrix_bytes(r0, idx, palette).tobytes())
    return dict(sample_ids=sample_ids, kind=kind)
