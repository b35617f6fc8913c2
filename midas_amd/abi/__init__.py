"""ctypes binding of include/midas_snps.h (libmidas_snps_hip.so).

There is no CPU fallback: if the library is missing, or no gfx950 GPU is visible,
the calls raise.  Nothing under ``oracle/`` is imported from here.

This file is the facade: every name lives in the module of its command family (core, reads, pileup, merge, genes, sites,
species, comm), each with its signature table, constants and wrappers; context.py puts Context together.
"""

from .core import (ABI_VERSION, ERR_BAD_LAYOUT, ERR_HIP, ERR_INVALID_ARG, ERR_NO_DEVICE, ERR_OUT_OF_MEMORY, ERR_READ_BAD_CIGAR_OP,
                   ERR_READ_CIGAR_OVERRUN, ERR_READ_NO_NM, ERR_READ_NO_QUAL, ERR_READ_NO_SEQ, ERR_READ_ZERO_ALIGN, ERR_UNSUPPORTED,
                   MidasSnpsError, PinnedPool, _Column, _GenesOwner, library_path, load_library, mt_states, symbols)
from .reads import (SAM_ORDERS, SAM_PHASES, BamDeviceHandle, BamShare, BamSlice, ContigTable, ReadsSoA, ResidentReads, _BamOwner, _Contigs,
                    _FastaOwner, _Reads, _SOA_DTYPES, _bam_columns, _bam_refs, open_bam_device, read_bam, read_fasta_files, read_sam,
                    sam_decode_timing, write_bam)
from .pileup import (DEFAULT_ARGS, INDEX_FACTS, NUM_STATS, PAD_PYSAM, PAD_SPEC, PATH_AUTO, PATH_DIRECT, PATH_LONG, PATH_NAMES, PATH_PACKED,
                     ROWS_DEVICE, ROWS_HOST, ROWS_PER_MEMBER, STAT_ALIGNED_READS, STAT_COVERED_BASES, STAT_MAPPED_READS, STAT_TOTAL_DEPTH,
                     Batch, BatchInfo, Thresholds, count_snps_rows, deflate_rows, read_snps_counts, read_snps_table, write_rows,
                     write_table)
from .merge import (DEFAULT_MERGE_ARGS, ERR_MERGE_ZERO_MEAN_DEPTH, GENES_MATRIX_KINDS, SNP_TYPE_BITS, SNP_TYPE_NAMES, TABLES_READ_PHASES,
                    TABLES_READ_STATS, GeneClusterMap, GeneTables, MergeParams, MergeTables, _Genes, format_repr_f64, write_genes_matrix,
                    write_merge_info, write_merge_matrix, write_merge_matrix_device)
from .genes import GENES_BAM_PHASES, GENES_BAM_STATS, GENES_DISTANCES, GENES_DTYPES, GenesMatrix, genes_curves, pandas_cell
from .sites import (ALLELE_LETTERS, SITES_LD_MAX_BINS, SITES_LD_SAME_GENE, SITES_MASK_ONLY, SITES_MAX_CLASSES, SITES_PAIR_TILE,
                    SITES_PER_GENE, SITES_POOLED, SITES_ROUND, SITES_SEQ, SITES_SUMS, SITES_WEIGHT, SitesTables, parse_cell)
from .species import (SPECIES_MERGE_PHASES, SPECIES_MERGE_REASONS, SPECIES_MERGE_STATS, SPECIES_PHASES, SPECIES_REASONS, SpeciesMerge,
                      species_assign, species_parse_number)
from .comm import Comm
from .context import Context

# every entry point is declared once, in its family's module; the lists are what the families registered
EXPORTED_SYMBOLS, SITES_SYMBOLS, TREE_SYMBOLS, SPECIES_SYMBOLS, SPECIES_MERGE_SYMBOLS, SAM_SYMBOLS = (
    symbols(tag) for tag in ('exported', 'sites', 'tree', 'species', 'species_merge', 'sam'))
