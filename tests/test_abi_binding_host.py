"""The binding package midas_amd/abi held against its own past and against include/midas_snps.h (no GPU needed):
the surface every caller imports, the symbol lists against the header's declarations, and every argtypes' length against the
header's parameter count."""
import inspect
import itertools
import os
import re

import numpy as np

from midas_amd import abi
from midas_amd.analyze import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# every public attribute of the binding when it was one module (imports left out), and the underscore names callers use
NAMES = '''
ABI_VERSION ALLELE_LETTERS BamDeviceHandle BamShare BamSlice Batch BatchInfo Comm Context ContigTable DEFAULT_ARGS
DEFAULT_MERGE_ARGS ERR_BAD_LAYOUT ERR_HIP ERR_INVALID_ARG ERR_MERGE_ZERO_MEAN_DEPTH ERR_NO_DEVICE ERR_OUT_OF_MEMORY
ERR_READ_BAD_CIGAR_OP ERR_READ_CIGAR_OVERRUN ERR_READ_NO_NM ERR_READ_NO_QUAL ERR_READ_NO_SEQ ERR_READ_ZERO_ALIGN
ERR_UNSUPPORTED EXPORTED_SYMBOLS GENES_BAM_PHASES GENES_BAM_STATS GENES_DISTANCES GENES_DTYPES GENES_MATRIX_KINDS
GeneClusterMap GeneTables GenesMatrix INDEX_FACTS MergeParams MergeTables MidasSnpsError NUM_STATS PAD_PYSAM PAD_SPEC
PATH_AUTO PATH_DIRECT PATH_LONG PATH_NAMES PATH_PACKED PinnedPool ROWS_DEVICE ROWS_HOST ROWS_PER_MEMBER ReadsSoA
ResidentReads SAM_ORDERS SAM_PHASES SAM_SYMBOLS SITES_LD_MAX_BINS SITES_LD_SAME_GENE SITES_MASK_ONLY SITES_MAX_CLASSES
SITES_PAIR_TILE SITES_PER_GENE SITES_POOLED SITES_ROUND SITES_SEQ SITES_SUMS SITES_SYMBOLS SITES_WEIGHT SNP_TYPE_BITS
SNP_TYPE_NAMES SPECIES_MERGE_PHASES SPECIES_MERGE_REASONS SPECIES_MERGE_STATS SPECIES_MERGE_SYMBOLS SPECIES_PHASES
SPECIES_REASONS SPECIES_SYMBOLS STAT_ALIGNED_READS STAT_COVERED_BASES STAT_MAPPED_READS STAT_TOTAL_DEPTH SitesTables
SpeciesMerge TABLES_READ_PHASES TABLES_READ_STATS TREE_SYMBOLS Thresholds _BamOwner _Contigs _Genes _Reads _SOA_DTYPES
_bam_columns _bam_refs count_snps_rows deflate_rows format_repr_f64 library_path load_library mt_states open_bam_device
pandas_cell parse_cell read_bam read_fasta_files read_sam read_snps_counts read_snps_table sam_decode_timing species_assign
species_parse_number write_bam write_genes_matrix write_merge_info write_merge_matrix write_merge_matrix_device write_rows
write_table
'''.split()

# str(inspect.signature()) of every public method of Context and Batch (and __init__), annotations left out: names and defaults
SIGNATURES = {
    'Context.__init__': '(self, device=0)',
    'Context.batch': '(self, contigs, reads)',
    'Context.calibration_pass': '(self, nbytes=1073741824)',
    'Context.close': '(self)',
    'Context.copy_rate': '(self, nbytes=1073741824, reps=10)',
    'Context.device_info': '(self)',
    'Context.fetch_payload': '(self, reads)',
    'Context.genes_assoc': "(self, text, n_rows, n_samples, n_columns, use, case, planes, cutoff=0.35, dtype='presabs', min_present=1, "
                           "min_absent=0, group_rows=0, chunk_bytes=0, form=1, products=False)",
    'Context.genes_compare': "(self, text, n_rows, n_samples, n_columns, dtype='presabs', distance='jaccard', cutoff=0.35, group_rows=0, "
                             "chunk_bytes=0, pair_blocks=0, dump=False)",
    'Context.genes_count': '(self, thr, reads, ref_id, gene_length)',
    'Context.genes_count_bam': '(self, thr, handle, gene_length)',
    'Context.genes_count_bam_timing': '(self)',
    'Context.genes_count_device': '(self, thr, reads, ref_id, gene_length)',
    'Context.genes_count_timing': '(self)',
    'Context.genes_linkage': '(self, text, n_rows, n_samples, n_columns, need, cutoff=0.35, min_present=2, min_absent=2, '
                             'max_pairs=67108864, group_rows=0, chunk_bytes=0, pair_form=0, pair_out=None)',
    'Context.genes_merge': '(self, cluster, copy, depth, reads, n_clusters, min_copy, group_samples=0)',
    'Context.genes_sum': '(self, gene, term, n_genes)',
    'Context.genes_terms': '(self, thr, reads, ref_id, gene_length)',
    'Context.inflate_blocks': '(self, comp, cpos, clen, upos, ulen, out_bytes, crc=None)',
    'Context.merge_sites': '(self, prm, sample_counts, mean_depth)',
    'Context.merge_sites_tables': '(self, prm, sample_counts, mean_depth, freq_path, depth_path, header_line, site_id_base=0)',
    'Context.mt19937_stream': '(self, key, pos, n_words, per_launch=0, bound=4294967295)',
    'Context.nj_tree': '(self, dist)',
    'Context.parse_rows': '(self, text, skip_header=True, cap_rows=None)',
    'Context.pileup': '(self, thr, contigs, reads, want_allele=True, pinned_slot=None)',
    'Context.pinned': '(self, key, shape, dtype)',
    'Context.read_snps_counts_device': '(self, paths, row_begin=0, max_rows=-1, first_slot=0, extra_slots=0)',
    'Context.row_coder_counts': '(self)',
    'Context.rows_code': '(self, counts, allele, members, arena_bytes=0, grid_blocks=0)',
    'Context.scan_u32': '(self, v, in_place=False, n=None)',
    'Context.set_default_path': '(self, path)',
    'Context.set_pad_rule': '(self, rule)',
    'Context.set_row_coder': '(self, coder)',
    'Context.set_stream': '(self, hip_stream)',
    'Context.sites_consensus_pairs': '(self, freq_text, depth_text, site_mask, sample_col, mean_depth, site_depth, site_ratio, '
                                     'allele_support, site_prev, site_maf, max_sites=-1, flags=0, group_rows=0, chunk_bytes=0, '
                                     'pair_blocks=0)',
    'Context.sites_id_markers': '(self, freq_text, depth_text, minor_code, major_code, sample_col, min_freq, min_reads, allele_prev, '
                                'n_parse=None, group_rows=0, chunk_bytes=0)',
    'Context.sites_ld': '(self, freq_text, depth_text, site_mask, sample_col, mean_depth, site_key, site_gene, site_depth, site_ratio, '
                        'allele_support, site_prev, site_maf, max_dist=1000, bin_width=10, min_samples=4, max_sites=-1, flags=0, '
                        'group_rows=0, chunk_bytes=0, anchor_chunk=0)',
    'Context.sites_pair_diversity': '(self, freq_text, depth_text, site_mask, sample_col, mean_depth, site_depth, site_ratio, '
                                    'allele_support, site_prev, site_maf, snp_maf=0.01, max_sites=-1, flags=0, group_rows=0, '
                                    'chunk_bytes=0, pair_form=0)',
    'Context.sites_scan': '(self, freq_text, depth_text, site_mask, sample_col, mean_depth, site_depth, site_ratio, allele_support, '
                          'site_prev, site_maf, snp_maf=0.01, max_sites=-1, flags=0, site_gene=None, n_genes=0, minor=None, major=None, '
                          'group_rows=0, chunk_bytes=0, dump=False, dump_keep=False, rand_reads=0, replace_reads=False, np_state=None, '
                          'draw_chunk=0, _classes=None)',
    'Context.sites_scan_classes': '(self, freq_text, depth_text, site_mask, site_class, n_classes, sample_col, mean_depth, site_depth, '
                                  'site_ratio, allele_support, site_prev, site_maf, **kw)',
    'Context.sites_track_markers': '(self, freq_text, depth_text, site_which, sample_col, min_freq, min_reads, n_parse=None, '
                                   'group_rows=0, chunk_bytes=0, pair_blocks=0)',
    'Context.sort_pairs': '(self, key, val, bits, n=None)',
    'Context.species_classify': '(self, text, gene_names, gene_species, gene_marker, n_species, marker_cutoff, aln_cov, chunk_bytes=0, '
                                'hash_bits=0, dump=False)',
    'Context.species_merge': '(self, profile_paths, species_ids, sample_depth=1.0, chunk_bytes=0, lds_bound=0, threads=0)',
    'Context.stream_rates': '(self, nbytes=4294967296, reps=5)',
    'Batch.__init__': '(self, ctx, contigs, reads)',
    'Batch.close': '(self)',
    'Batch.enable_timing': '(self, n_slots=1)',
    'Batch.fetch': '(self, counts=True, allele=True, stats=True)',
    'Batch.fetch_index': '(self)',
    'Batch.fetch_packed': '(self)',
    'Batch.info': '(self)',
    'Batch.last_timing': '(self)',
    'Batch.pack': '(self)',
    'Batch.pack_timing': '(self, slot=0)',
    'Batch.run': '(self, thr)',
    'Batch.select_path': '(self, path)',
    'Batch.stats_to_device': '(self, dst_device_ptr)',
    'Batch.sync': '(self)',
    'Batch.time_pileup_only': '(self, on=True)',
    'Batch.timing': '(self, slot=0)',
    'Batch.write_part': '(self, path, contig_index, ref_ids, header=True, gz_level=4, threads=0)',
}

SYMBOL_LISTS = ('EXPORTED_SYMBOLS', 'SITES_SYMBOLS', 'TREE_SYMBOLS', 'SPECIES_SYMBOLS', 'SPECIES_MERGE_SYMBOLS', 'SAM_SYMBOLS')


def _header():
    src = open(os.path.join(ROOT, "include", "midas_snps.h")).read()
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S))


def _bound():
    return [sym for name in SYMBOL_LISTS for sym in getattr(abi, name)]


def _plain_signature(fn) -> str:
    sig = inspect.signature(fn)
    empty = inspect.Parameter.empty
    return str(sig.replace(parameters=[p.replace(annotation=empty) for p in sig.parameters.values()], return_annotation=empty))


def test_every_name_callers_use_is_on_the_package():
    missing = [n for n in NAMES if not hasattr(abi, n)]
    assert not missing, missing


def test_context_and_batch_methods_keep_names_and_defaults():
    now = {}
    for cls in (abi.Context, abi.Batch):
        for name, fn in inspect.getmembers(cls, callable):
            if not name.startswith('_') or name == '__init__':
                now['%s.%s' % (cls.__name__, name)] = _plain_signature(fn)
    assert sorted(now) == sorted(SIGNATURES)
    wrong = {k: (now[k], v) for k, v in SIGNATURES.items() if now[k] != v}
    assert not wrong, wrong


def test_symbol_lists_partition_the_header():
    declared = set(re.findall(r"\b(midas_[a-z_0-9]+)\s*\(", _header()))
    lists = {name: set(getattr(abi, name)) for name in SYMBOL_LISTS}
    for a, b in itertools.combinations(SYMBOL_LISTS, 2):
        assert not lists[a] & lists[b], (a, b, lists[a] & lists[b])
    bound = _bound()
    assert len(bound) == len(set(bound))
    assert set(bound) == declared, (sorted(set(bound) - declared), sorted(declared - set(bound)))
    prefixes = ('midas_snps_', 'midas_bam_', 'midas_merge_', 'midas_genes_', 'midas_comm_', 'midas_fasta_')
    assert lists['EXPORTED_SYMBOLS'] == {s for s in declared if s.startswith(prefixes)}
    lib = abi.load_library()
    assert all(getattr(lib, sym).argtypes is not None for sym in bound)


def test_every_argtypes_has_the_header_s_parameter_count():
    header = _header()
    lib = abi.load_library()
    wrong = {}
    for sym in _bound():
        m = re.search(r"\b%s\s*\(([^()]*)\)\s*;" % sym, header)
        assert m, "%s: its declaration is not of the form NAME(parameters);" % sym
        params = m.group(1).strip()
        want = 0 if params in ('', 'void') else params.count(',') + 1
        if len(getattr(lib, sym).argtypes) != want:
            wrong[sym] = (len(getattr(lib, sym).argtypes), want)
    assert not wrong, wrong


def test_sites_tables_column_hands_out_what_strings_reads(tmp_path):
    """SitesTables.column: no command calls it; the smallest directory (2 samples, 3 sites), every string column."""
    d = str(tmp_path / "species_1")
    synth.write_species_dir(d, 3, 2, seed=1)
    t = abi.SitesTables(d)
    assert (t.n_sites, t.n_columns) == (3, 2)
    for name in t.STRING_COLUMNS:
        pool, off = t.column(name)
        assert pool.dtype == np.uint8 and off.dtype == np.int64 and off[0] == 0 and off[-1] == pool.shape[0]
        assert [pool[int(off[k]):int(off[k + 1])].tobytes().decode() for k in range(off.shape[0] - 1)] == t.strings(name)
    assert t.column('site_id')[1].shape == (4,) and t.column('matrix_sample_id')[1].shape == (3,)
