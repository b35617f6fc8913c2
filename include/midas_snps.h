/*
 * midas_snps.h -- C-ABI of the MI355X-native MIDAS SNP pileup (libmidas_snps_hip.so).
 *
 * This is the drop-in boundary for ONE path of snayfach/MIDAS: the pileup +
 * allele-count stage of `run_midas.py snps`.  The reference has no FFI for it;
 * the seam is Python (all citations are into /root/reference):
 *
 *   midas/run/snps.py:301      pysam_pileup(args, species, contigs)
 *   midas/run/snps.py:194-199  bamfile.count_coverage(contig.id, start=0, end=contig.length,
 *                                quality_threshold=args['baseq'], read_callback=keep_read)
 *   midas/run/snps.py:141-162  keep_read(aln)                  (per-read filter + 2 counters)
 *   midas/run/snps.py:201-213  per-site emit loop              (ref_allele, depth, 3 counters)
 *   midas/run/snps.py:130-137  index_bam                       (samtools index)
 *
 * Every entry point below names the reference line(s) it replaces.  Only plain C
 * types cross the boundary.  Ownership: the caller allocates and owns every host
 * buffer it passes in or receives results in; the library never keeps a host
 * pointer past the call that received it and never frees caller memory.  Device
 * memory is owned by the context / batch objects and released by their destroy
 * calls.  No global state; a context is bound to one GPU and may be used by one
 * thread at a time (use one context per thread / per rank).
 *
 * Error convention: every call returns MIDAS_SNPS_OK (0) or a negative /
 * positive status; midas_snps_last_error() returns a human-readable message for
 * the last failing call on that context.  Nothing aborts or throws across the
 * ABI.  The Python host turns a non-zero status into the reference's own
 * convention, sys.exit("\nError: ...\n") (midas/utility.py:227-232).
 *
 * There is NO CPU fallback behind these symbols: if no gfx950 device is present
 * midas_snps_create() fails with MIDAS_SNPS_ERR_NO_DEVICE.  The host-only
 * helpers (pack / plan / version) work without a GPU.
 */
#ifndef MIDAS_SNPS_H
#define MIDAS_SNPS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MIDAS_SNPS_ABI_VERSION 4      /* 4: midas_snps_batch_info grew by direct_chunk_tiles, direct_overhang */

/* ---- status codes ------------------------------------------------------- */
enum {
  MIDAS_SNPS_OK = 0,
  /* Per-read conditions under which the reference raises inside the worker
   * (numbering shared with oracle/pileup_oracle.py).  The offending read index
   * (lowest one) is in the error string and in midas_snps_last_error_read(). */
  MIDAS_SNPS_ERR_READ_NO_SEQ = 1,        /* len(aln.query_alignment_sequence) on None: TypeError  (snps.py:145) */
  MIDAS_SNPS_ERR_READ_NO_NM = 2,         /* dict(aln.tags)['NM']: KeyError                         (snps.py:148) */
  MIDAS_SNPS_ERR_READ_ZERO_ALIGN = 3,    /* /float(align_len) with align_len == 0: ZeroDivisionError (snps.py:148) */
  MIDAS_SNPS_ERR_READ_NO_QUAL = 4,       /* np.mean(None): TypeError                               (snps.py:151) */
  MIDAS_SNPS_ERR_READ_CIGAR_OVERRUN = 5, /* seq[qpos] past l_seq on a kept read: IndexError        (pysam count_coverage) */
  MIDAS_SNPS_ERR_READ_BAD_CIGAR_OP = 6,  /* CIGAR op code > 8                                      */
  /* Library / argument errors */
  MIDAS_SNPS_ERR_INVALID_ARG = -1,
  MIDAS_SNPS_ERR_NO_DEVICE = -2,         /* no HIP device / not gfx950 / HIP runtime failure at create */
  MIDAS_SNPS_ERR_HIP = -3,               /* a HIP runtime call failed (message has hipGetErrorString) */
  MIDAS_SNPS_ERR_OUT_OF_MEMORY = -4,
  MIDAS_SNPS_ERR_UNSUPPORTED = -5,       /* a batch beyond what one batch addresses: > 2*10^9 reads, > 32 GiB of read payload
                                            (the caller splits it); baseq > 62 on a PACKED batch holding qualities above 62;
                                            selecting the DIRECT / PACKED path on a batch that holds a read beyond their
                                            limits (l_seq > 1024, n_cigar / NM > 65534: such a batch RUNS, on the long path);
                                            a contig of length < 1 (pysam: "interval of size 0") or >= 2^31 (BAM's limit)     */
  MIDAS_SNPS_ERR_BAD_LAYOUT = -6         /* offsets out of range / not monotone, read_begin inconsistent */
};

/* ---- thresholds: the five `args[...]` values the path reads --------------
 * scripts/run_midas.py:410-419 (defaults mapid 94.0, mapq 20, baseq 30, readq 20,
 * aln_cov 0.75); consumed at midas/run/snps.py:148-157 and :198.               */
typedef struct midas_snps_thresholds {
  int32_t baseq;    /* count a base iff qual >= baseq (baseq <= 0: every base)   */
  int32_t mapq;     /* keep read iff mapq >= mapq                                 */
  int32_t readq;    /* keep read iff mean(qual over all l_seq bases) >= readq     */
  int32_t reserved; /* must be 0                                                  */
  double mapid;     /* keep read iff 100*(align_len-NM)/float(align_len) >= mapid */
  double aln_cov;   /* keep read iff align_len/float(l_seq) >= aln_cov            */
} midas_snps_thresholds;

/* ---- inputs ---------------------------------------------------------------
 * Alignment records in BAM-native encodings, struct-of-arrays, host memory,
 * grouped by contig in the order of the contig table and (for speed, not for
 * correctness) sorted by pos inside a contig -- i.e. the order of the
 * coordinate-sorted snps/temp/genomes.bam (midas/run/snps.py:116-120).
 *   seq4:  4-bit codes "=ACMGRSVTWYHKDBN", two per byte, first base in the high nibble
 *   qual:  phred bytes, l_seq per read; qual[0]==0xFF means QUAL absent
 *   cigar: u32 = len<<4 | op, op in MIDNSHP=X (0..8)
 *   nm:    NM aux tag, or -1 when the record has none
 *   *_off: CSR offsets, n_reads+1 entries each (seq_off/qual_off in bytes, cigar_off in u32 elements)
 * `flag` is carried for completeness; the path never looks at it (with a callable
 * read_callback pysam applies no flag filter), and it may be NULL.               */
typedef struct midas_snps_reads {
  int64_t n_reads;
  const int32_t* pos;
  const uint8_t* mapq;
  const uint16_t* flag;
  const int32_t* nm;
  const int32_t* l_seq;
  const int64_t* seq_off;
  const int64_t* qual_off;
  const int64_t* cigar_off;
  const uint8_t* seq4;        /* these three: host memory, or memory of the context's device (midas_bam_load_device leaves  */
  const uint8_t* qual;        /* them there) -- all three alike; midas_snps_batch_create / midas_snps_pileup copy either way;     */
  const uint32_t* cigar;      /* the host-only entry points (midas_snps_write_*, midas_genes_count / _terms) take host memory only;   */
                              /* midas_genes_count_device takes qual / cigar on the device                                            */
} midas_snps_reads;

/* Contig table: what initialize_contigs() builds (midas/run/snps.py:55-67), flattened.
 * `ref` holds the FASTA letters of all contigs back to back in table order (any case;
 * the library upper-cases ASCII a-z exactly like str.upper() at snps.py:62).
 * Reads of contig c are read indices [read_begin[c], read_begin[c+1]).            */
typedef struct midas_snps_contigs {
  int32_t n_contigs;
  int32_t n_species;
  const int64_t* length;      /* [n_contigs]   > 0                                  */
  const int32_t* species;     /* [n_contigs]   species index in [0, n_species)      */
  const int64_t* read_begin;  /* [n_contigs+1] non-decreasing, last == n_reads      */
  const uint8_t* ref;         /* [sum(length)]                                      */
  /* NULL, or [n_contigs]: entry c is a PIECE of a longer contig, starting at its 0-based position origin[c] (0: the contig's
   * start).  A long contig can then be piled up piece by piece -- on different GPUs -- and the pieces' tables concatenated
   * (midas_snps_write_part takes the position its rows start at).  `length`, `ref` and the read positions are the piece's:
   * pos is relative to origin[c] and NEGATIVE for a read that starts in front of the piece and reaches into it -- such a
   * read is tallied where it covers the piece, but with origin[c] > 0 it is the PREVIOUS piece's read: it is not counted in
   * aligned_reads / mapped_reads here and what keep_read would raise for it is not reported here (its own piece does both;
   * a CIGAR that overruns SEQ at a site of THIS piece is reported here, where the walk meets it).
   * count_coverage is called per contig at midas/run/snps.py:194-199; the split is this library's.                       */
  const int64_t* origin;
} midas_snps_contigs;

/* Per-species counters, in this order (midas/run/snps.py:172-176, 211-213, 143, 161).
 * genome_length is sum(length) and is left to the caller.                          */
enum {
  MIDAS_SNPS_STAT_ALIGNED_READS = 0,
  MIDAS_SNPS_STAT_MAPPED_READS = 1,
  MIDAS_SNPS_STAT_COVERED_BASES = 2,
  MIDAS_SNPS_STAT_TOTAL_DEPTH = 3,
  MIDAS_SNPS_NUM_STATS = 4
};

typedef struct midas_snps_ctx midas_snps_ctx;
typedef struct midas_snps_batch midas_snps_batch;

/* ---- library ------------------------------------------------------------ */
int32_t midas_snps_abi_version(void);
/* Host threads the library's parallel regions use (BAM inflate / decode, row formatting + gzip, table parsing): the CPUs the
 * process may run on -- hardware threads, its affinity mask, a cgroup CPU quota, whichever is least -- divided by
 * LOCAL_WORLD_SIZE under torchrun.  Replaces the `threads` argument of utility.parallel's mp.Pool (midas/utility.py:81-107). */
int32_t midas_snps_cpu_budget(void);
/* Static string for a status code (never NULL). */
const char* midas_snps_status_string(int32_t status);

/* ---- context: one per GPU ------------------------------------------------
 * Replaces the per-worker-process module globals `aln_stats` / `global_args`
 * (midas/run/snps.py:142,167-176) and the mp.Pool worker itself
 * (midas/utility.py:81-107).                                                     */
int32_t midas_snps_create(int32_t device_ordinal, midas_snps_ctx** out_ctx);
void midas_snps_destroy(midas_snps_ctx* ctx);
const char* midas_snps_last_error(const midas_snps_ctx* ctx);
/* Lowest index of a read that made the last pileup fail with a MIDAS_SNPS_ERR_READ_* status, else -1. */
int64_t midas_snps_last_error_read(const midas_snps_ctx* ctx);
/* Launch on an existing HIP stream (hipStream_t as void*; e.g. torch's current stream) instead of
 * the context's own.  NULL restores the context's stream -- so HIP's null (legacy default) stream
 * cannot be named here: a caller whose framework runs on the default stream (torch.cuda.current_stream()
 * has the handle 0 until a stream is made current) makes a stream of its own current and passes that
 * one, as bench.py does; otherwise the framework's copies and collectives do not wait for this
 * library's kernels.                                                                             */
int32_t midas_snps_set_stream(midas_snps_ctx* ctx, void* hip_stream);
/* Device facts for logs: name (<=255 chars), compute units, HBM bytes. */
int32_t midas_snps_device_info(const midas_snps_ctx* ctx, char* name256, int32_t* n_cu, int64_t* hbm_bytes);

/* What a plain device-to-device copy reaches on this device right now, in GB/s (bytes read + bytes written per second):
 * `reps` passes of the library's own 16-bytes-per-lane copy kernel over `bytes` (>= 1 MiB), timed with HIP events.  The
 * practical HBM ceiling the roofline fractions of bench.py are also held against (measurement aid; no reference counterpart). */
int32_t midas_snps_copy_rate(midas_snps_ctx* ctx, int64_t bytes, int32_t reps, double* out_gbps);
/* The same question asked properly: a read stream, a write stream and a copy over `bytes` per buffer (use >= 4 GiB: far
 * beyond the 256 MiB Infinity Cache), `reps` passes each, by kernels built to saturate the memory pipe (a persistent grid
 * of 4 workgroups per CU, 16 bytes per lane, four independent accesses in flight).  out_gbps[0] bytes read per second by the
 * read stream, [1] bytes written per second by the write stream, [2] bytes read + written per second by the copy.  bench.py
 * quotes the largest of them as this box's ceiling (measurement aid; no reference counterpart).                       */
int32_t midas_snps_stream_rates(midas_snps_ctx* ctx, int64_t bytes, int32_t reps, double out_gbps[3]);
/* Counter calibration for rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE: reads `bytes` once with 4-, 8- and 16-byte-per-lane
 * loads and writes them once with 16-byte stores, one kernel each (midas_calib_read4_kernel, _read8_, _read16_,
 * midas_calib_write16_kernel): the counter value of each against the bytes it is known to move is the factor bench.py
 * applies to a product kernel with that access width (measurement aid; no reference counterpart).                     */
int32_t midas_snps_calibration_pass(midas_snps_ctx* ctx, int64_t bytes);

/* Page-locked host memory (hipHostMalloc).  Optional: every entry point takes ordinary memory; result buffers that come
 * from here are filled by one DMA instead of through the context's staging ring, and a caller that keeps them for the
 * lifetime of its context pays the pinning once.  NULL when no device / out of memory.                            */
void* midas_snps_host_alloc(int64_t bytes);
void midas_snps_host_free(void* ptr);

/* ---- one-shot: host buffers in, host buffers out --------------------------
 * Replaces, for every contig of the table at once, the call
 *   bamfile.count_coverage(contig.id, 0, contig.length, args['baseq'], keep_read)
 * (midas/run/snps.py:194-199) together with keep_read (:141-162) and the counter
 * part of the emit loop (:204-213).
 *   out_counts [sum(length) * 4] u32, per site A,C,G,T      (counts[0..3][i], :205-208)
 *   out_allele [sum(length)]     u8, upper-cased ref letter  (contig.seq[i],   :203) -- may be NULL
 *   out_stats  [n_species * 4]   i64, MIDAS_SNPS_STAT_* order
 * On a MIDAS_SNPS_ERR_READ_* status the outputs are unspecified, as in the
 * reference where the worker's exception discards them.                           */
int32_t midas_snps_pileup(midas_snps_ctx* ctx, const midas_snps_thresholds* thr,
                          const midas_snps_contigs* contigs, const midas_snps_reads* reads,
                          uint32_t* out_counts, uint8_t* out_allele, int64_t* out_stats);

/* ---- resident batches: upload once, run many ------------------------------
 * A batch is the device-resident form of (contig table, reads): the caller's BAM-native arrays
 * are uploaded as they are, every read is validated on the device, and the DIRECT layout is built from
 * them once -- one 16-byte record per read (pos, l_seq, n_cigar, NM, mapq, payload offset) and the read's
 * CIGAR / SEQ / QUAL bytes as one run of a payload in BAM's own order: columns re-encoded and bytes
 * gathered, nothing decided -- next to the reference letters and the tile table.  (The PACKED layout,
 * tile-ordered records + one byte per base, is built on first use: unsorted input, coverage hot spots.)
 * Creating it replaces what `pysam.AlignmentFile(bampath)` + htslib's record decode do per worker
 * (midas/run/snps.py:186); running it replaces index_bam (:130-137, the device
 * builds its own per-tile read index each run) and the calls named above.      */
int32_t midas_snps_batch_create(midas_snps_ctx* ctx, const midas_snps_contigs* contigs,
                                const midas_snps_reads* reads, midas_snps_batch** out_batch);
void midas_snps_batch_destroy(midas_snps_batch* batch);
/* The device paths of a batch.  DIRECT: the pileup kernel reads a read's 16-byte record and its BAM-order payload -- 4-bit
 * SEQ, QUAL, CIGAR as the BAM holds them -- and visits every read once: a pass over the positions alone (4 bytes per
 * read) finds, per 2048-site tile, the run of reads that can touch it; the kernel decides in registers what a read's CIGAR
 * is and tallies it; nothing is sorted or decided beforehand.  It wants position-sorted reads (what samtools sort
 * writes; any order is CORRECT, only slower).  PACKED: the reads are first laid out in tile order as records + one byte per
 * base (midas_snps_batch_pack), which handles any order and cuts coverage hot spots into parts.  batch_create picks DIRECT
 * unless the reads are badly ordered, one read spans many tiles or a tile holds a hot spot; AUTO restores that choice.
 * Both paths give bit-identical results (tests/test_gpu_direct.py).  LONG: a batch that holds a read beyond the two fast
 * paths' limits -- l_seq above 1024, more than 65 534 CIGAR ops, NM above 65 534; pysam knows no such limits
 * (midas/run/snps.py:187-199) -- is not refused: batch_create gives it the long path (pileup_long.hip: one thread per read,
 * op by op and base by base from the caller's arrays, global atomics, the ratio tests in fp64), exact and slow, the only
 * path such a batch has (selecting DIRECT or PACKED on it is MIDAS_SNPS_ERR_UNSUPPORTED; any batch may select LONG).      */
enum { MIDAS_SNPS_PATH_AUTO = 0, MIDAS_SNPS_PATH_DIRECT = 1, MIDAS_SNPS_PATH_PACKED = 2, MIDAS_SNPS_PATH_LONG = 3 };
int32_t midas_snps_batch_select_path(midas_snps_batch* batch, int32_t path);
/* The path of every batch created on the context from now on (the one-shot midas_snps_pileup included); AUTO = each
 * batch's own choice.                                                                                              */
int32_t midas_snps_set_default_path(midas_snps_ctx* ctx, int32_t path);
/* What the CIGAR op P (padding) does to the QUERY position in the walk behind count_coverage ([EXT] pysam
 * get_aligned_pairs(matches_only=True), reached from midas/run/snps.py:194-199):
 *   MIDAS_SNPS_PAD_SPEC   (default) nothing -- the SAM specification: P consumes neither query nor reference; the worked
 *                         example of SAMv1 section 1.1 (read r002, 3S6M1P1I4M) only comes out as printed under this rule;
 *   MIDAS_SNPS_PAD_PYSAM  the query advances, as get_aligned_pairs of the pysam releases of MIDAS's time does (BAM_CPAD sits
 *                         in the branch of BAM_CINS / BAM_CSOFT_CLIP there): bases behind a pad are read one position late and
 *                         a read whose last match op then runs past SEQ inside the contig raises IndexError when kept
 *                         (MIDAS_SNPS_ERR_READ_CIGAR_OVERRUN here).
 * bowtie2 -- the only aligner run_midas.py snps drives -- never writes P, so the two rules give the same tables on every BAM
 * the reference itself produces; the switch exists because bit-identity is promised against the dependency, whose behaviour on
 * this op cannot be pinned in an image without pysam.  Clip lengths (query_alignment_start / _end) never look at P.  Applies
 * to batches created on the context afterwards (the one-shot midas_snps_pileup included).                              */
enum { MIDAS_SNPS_PAD_SPEC = 0, MIDAS_SNPS_PAD_PYSAM = 1 };
int32_t midas_snps_set_pad_rule(midas_snps_ctx* ctx, int32_t rule);
/* Who formats and deflates the rows midas_snps_batch_write_part writes at gz levels 1-5 (the row coder's levels):
 *   MIDAS_SNPS_ROWS_DEVICE (default)  a kernel, one workgroup per gzip member: what crosses the link is the DEFLATE stream
 *                                     (~4 bytes a row) and the host only frames and writes the members;
 *   MIDAS_SNPS_ROWS_HOST              the host's formatter threads, from counts and alleles streamed through the pinned ring
 *                                     (the file is then byte for byte what midas_snps_write_part writes).
 * Both give gzip files that inflate to the same text -- the rows of midas/run/snps.py:201-210 -- but not the same bytes: the
 * two coders choose their matches differently.  Every rank of a job uses the same coder, so parts still concatenate into the
 * file one rank writes.  The environment variable MIDAS_SNPS_ROW_CODER=host sets the default of new contexts.          */
enum { MIDAS_SNPS_ROWS_DEVICE = 0, MIDAS_SNPS_ROWS_HOST = 1 };
int32_t midas_snps_set_row_coder(midas_snps_ctx* ctx, int32_t coder);
/* Who coded the parts midas_snps_batch_write_part has written on this context at the row coder's levels since it was created:
 *   out3[0]  gzip members formatted and deflated by the kernel (counted when their part is in the file);
 *   out3[1]  parts left to the host's formatter before the launch: a contig id longer than the kernel's 192 bytes;
 *   out3[2]  parts left to it after the launch: a member came back with a status other than 0 (the arena was full).
 * A part is one midas_snps_batch_write_part call.  midas_snps_rows_code counts nothing here (test aid; no reference counterpart). */
int32_t midas_snps_row_coder_counts(const midas_snps_ctx* ctx, int64_t out3[3]);
/* The row kernel's launch of midas_snps_batch_write_part on inputs of the caller's choosing: counts [n_sites * 4] and allele
 * [n_sites] (any byte) go up, and member k -- rows site0[k] .. site0[k] + n_rows[k] - 1 of them, numbered from pos0[k], under the id
 * ids[id_off[k], + id_len[k]) -- is handed to the kernel as given, a member the product never forms included (an id beyond 192
 * bytes, no rows, more than 16 384): the kernel answers those with status 1.  Only what would read outside the arrays is refused
 * here (MIDAS_SNPS_ERR_INVALID_ARG): sites of a member the kernel takes that are not in [0, n_sites), positions that pass 2^31 - 1,
 * an id outside ids.  arena_bytes: the room for all streams together, 0 = the product's rule (10 bytes a row + 1 KiB a member +
 * 4 KiB); grid_blocks: workgroups of the launch (never more than members), 0 = one per compute unit, as the product launches.
 * Per member: out_status (0 coded; 1 not taken; 2 the arena was full), out_n_bytes, out_crc (CRC-32 of the member's text),
 * out_text_len (status 0 and 2), out_arena_off (where its stream lay in the arena; -1 unless status 0).  The raw DEFLATE streams
 * of the members with status 0 follow one another, in the members' order, in out_streams[0, *out_stream_bytes);
 * MIDAS_SNPS_ERR_INVALID_ARG when out_cap is too small (the arena's size always suffices).  Same code as the product's path
 * from the upload of the members to the streams' way down (test aid; no reference counterpart).                          */
int32_t midas_snps_rows_code(midas_snps_ctx* ctx, int64_t n_sites, const uint32_t* counts, const uint8_t* allele, int32_t n_members,
                             const int64_t* site0, const int64_t* pos0, const int32_t* n_rows, const int32_t* id_off,
                             const int32_t* id_len, const uint8_t* ids, int64_t ids_bytes, int64_t arena_bytes, int32_t grid_blocks,
                             uint32_t* out_status, uint32_t* out_n_bytes, uint32_t* out_crc, uint32_t* out_text_len,
                             int64_t* out_arena_off, uint8_t* out_streams, int64_t out_cap, int64_t* out_stream_bytes);
/* The library's two generic device primitives (device_sort.hip) on host arrays of the caller's choosing, through the launches
 * every front end uses (test aids; no reference counterpart).  The arrays go up, the launch runs on the context's stream, the result
 * comes down.  Every device buffer of a call lies between 64 guard words in front and 64 behind, written before the launch and
 * compared afterwards; the scan's sums and the sort's scratch are exactly as many words as the library's callers allocate.
 * *out_guards_ok: 1 when every guard word is as it was, else 0.  n == 0 is legal (nothing is written to the outputs but the flags).
 * MIDAS_SNPS_ERR_INVALID_ARG: a null context, n < 0, bits outside 0..32, a value_kind other than 0 and 1, a missing array.
 *
 * midas_snps_scan_u32: out[i] = (in[0] + ... + in[i - 1]) mod 2^32.  in_place != 0: one device buffer is both the scan's input
 * and its output; else two, and *out_in_kept says whether the input's buffer still held `in` after the launch (1 in place).   */
int32_t midas_snps_scan_u32(midas_snps_ctx* ctx, int64_t n, const uint32_t* in, int32_t in_place, uint32_t* out, int32_t* out_guards_ok,
                            int32_t* out_in_kept);
/* midas_snps_sort_pairs: the stable sort of (key[i], val[i]) by the low `bits` bits of the keys (keys must lie below 2^bits; n below
 * 2^32).  value_kind 0: val and out_val are uint32_t[n]; 1: double[n], moved as 64-bit patterns.  *out_which: the device buffer
 * pair the launch named as the result -- 0 the pair the input was uploaded to, 1 the other one.                             */
int32_t midas_snps_sort_pairs(midas_snps_ctx* ctx, int64_t n, int32_t bits, int32_t value_kind, const uint32_t* key, const void* val,
                              uint32_t* out_key, void* out_val, int32_t* out_which, int32_t* out_guards_ok);
/* midas_snps_mt19937_stream: the device's MT19937 generator (mt19937_stream.hip; snp_diversity.py --rand_reads) on host arrays
 * (test aid).  From numpy's legacy state (key624, pos 0 .. 624) n_words words are generated, per_launch a launch (0: one launch):
 * out_raw [n] the tempered words, out_flag [n] (nullable) 1 where (word & mask) <= bound with mask the smallest 2^j - 1 >= bound,
 * out_masked [n] (nullable) word & mask; out_key624 / out_pos: the state behind the last word.                                 */
int32_t midas_snps_mt19937_stream(midas_snps_ctx* ctx, const uint32_t* key624, int32_t pos, int64_t n_words, int64_t per_launch, int64_t bound,
                                  uint32_t* out_raw, uint8_t* out_flag, uint32_t* out_masked, uint32_t* out_key624, int32_t* out_pos);
/* Re-run the device packer over the batch's resident BAM-native arrays (the arrays batch_create uploaded, unchanged):
 * per read the CIGAR walk into gap-free match segments (pysam get_aligned_pairs(matches_only=True), reached from
 * midas/run/snps.py:194-199), the clip structure (query_alignment_sequence, :145), floor(mean(query_qualities))
 * (:151, a wave reduction), the 'A','C','G','T'-only rule folded into the quality bytes, and the tile order the
 * index kernel expects (:130-137).  batch_create already ran it once; this entry exists so that a caller can time
 * "raw reads resident in HBM -> counts" (pack + run).  Returns after the pack has finished (the hot-spot plan needs
 * the per-tile read counts on the host).                                                                          */
int32_t midas_snps_batch_pack(midas_snps_batch* batch);
/* Copy the packed device layout back (tests: it must equal the host mirror tests/mirror/pack_mirror.cpp bit for bit).
 * rec16 [(n_records+1)*16], blob [blob_bytes], orig_index / key [n_records]; any pointer may be NULL; the two sizes
 * are always returned.                                                                                            */
int32_t midas_snps_batch_fetch_packed(midas_snps_batch* batch, void* rec16, void* blob, uint32_t* orig_index,
                                      uint32_t* key, int64_t* out_n_records, int64_t* out_blob_bytes);
/* The direct path's index pass, looked at from outside (tests/test_gpu_index.py holds it to a model word for word): runs ONE
 * ranges pass on the batch's current parity exactly as a run on the direct path starts -- the same function: the ranges kernel,
 * then the listed outliers when the ranges keep to the common span -- advances the parity as a run does, and copies down
 *   tbegin, tend   [n_tiles]  the run of reads [tbegin, tend) every 2048-site tile streams (tbegin 0xFFFFFFFF: none reaches it);
 *   out_facts      [MIDAS_SNPS_INDEX_FACTS]  MIDAS_SNPS_INDEX_* order: the facts pass of batch_create as it was summed, and
 *                  what the batch derived from it;
 *   outliers3      [3 * n_outliers_listed]  (read, first tile, last tile) of every listed read that spans more than the
 *                  overhang, in the order the device listed them (any); never more than 3 * max(4096, n_reads / 64) words;
 *   tile_flag      [n_tiles]  1: an outlier leaves the tile's overhang here (such a tile's chunk is dealt tile by tile);
 *   chunk_ok       [*out_n_chunk_ok]  0: the chunk of four tiles holds a flagged tile; at most max(1, n_tiles / 4) bytes, and
 *                  *out_n_chunk_ok == 0 when the batch has no such table (every chunk carries its overhang, or no chunks).
 * Any output pointer may be NULL (chunk_ok only together with its length).  MIDAS_SNPS_ERR_INVALID_ARG: a null batch, chunk_ok
 * without out_n_chunk_ok; MIDAS_SNPS_ERR_UNSUPPORTED: a batch on the long path -- no ranges were ever built.  The per-species
 * counters of the last run are reset, as by a run: fetch results first (test aid; no reference counterpart).                 */
enum {
  MIDAS_SNPS_INDEX_STATUS = 0,        /* lowest (read << 8 | code) of a malformed read, -1 when every read is well-formed */
  MIDAS_SNPS_INDEX_ALG = 1,           /* sum(ceil(l/2) + l + 4 * n_cigar + 16)                                           */
  MIDAS_SNPS_INDEX_N_GENERAL = 2,
  MIDAS_SNPS_INDEX_N_LONG = 3,
  MIDAS_SNPS_INDEX_N_OUTLIERS = 4,    /* reads whose reference span exceeds the overhang                                  */
  MIDAS_SNPS_INDEX_MAX_L = 5,
  MIDAS_SNPS_INDEX_MAX_SPAN = 6,
  MIDAS_SNPS_INDEX_MAX_COMMON = 7,    /* longest reference span of a read that is no outlier                             */
  MIDAS_SNPS_INDEX_UNSORTED = 8,
  MIDAS_SNPS_INDEX_REACH = 9,
  MIDAS_SNPS_INDEX_REACH_RANGES = 10, /* what the ranges pass reaches back over                                          */
  MIDAS_SNPS_INDEX_OVERHANG = 11,     /* the overhang the facts pass judged the outliers by                              */
  MIDAS_SNPS_INDEX_CHUNKS = 12,
  MIDAS_SNPS_INDEX_N_LISTED = 13,
  MIDAS_SNPS_INDEX_OUTLIER_CAP = 14,
  MIDAS_SNPS_INDEX_FACTS = 15
};
int32_t midas_snps_batch_fetch_index(midas_snps_batch* batch, uint32_t* tbegin, uint32_t* tend, int64_t* out_facts, uint32_t* outliers3,
                                     uint8_t* tile_flag, uint8_t* chunk_ok, int64_t* out_n_chunk_ok);
/* Device-side durations of a timed pack (enable_timing slots, like batch_timing): [0] whole pack, [1] its scatter
 * kernel (the dominant one: raw reads in, records + payload out).                                                 */
int32_t midas_snps_batch_pack_timing(midas_snps_batch* batch, int32_t slot, float out_ms[2]);
/* Enqueue one full pass (index + filter + pileup + per-species counters) on the context's stream;
 * asynchronous.  Results stay on the device until midas_snps_batch_fetch().                    */
int32_t midas_snps_batch_run(midas_snps_batch* batch, const midas_snps_thresholds* thr);
/* Wait for the stream, then report the status of the last run (MIDAS_SNPS_ERR_READ_* possible). */
int32_t midas_snps_batch_sync(midas_snps_batch* batch);
/* sync + copy results to host.  Any of the three pointers may be NULL. */
int32_t midas_snps_batch_fetch(midas_snps_batch* batch, uint32_t* out_counts, uint8_t* out_allele,
                               int64_t* out_stats);
/* Facts about a batch, for roofline accounting: */
typedef struct midas_snps_batch_info {
  int64_t n_reads;
  int64_t n_sites;          /* sum(length)                                               */
  int64_t n_tiles;
  int64_t packed_bytes;     /* device bytes of packed records + payload                  */
  int64_t algorithmic_bytes;/* sum(ceil(l/2)+l+4*n_cigar+16) + 17*n_sites  */
  int32_t tile_sites;
  int32_t lanes_per_read;
  int64_t n_work_items;     /* >= n_tiles: a tile holding a coverage hot spot is processed as several parts */
  int32_t path;             /* MIDAS_SNPS_PATH_DIRECT / _PACKED / _LONG: what batch_run takes                 */
  int32_t path_auto;        /* what the batch's own numbers recommend (see midas_snps_batch_select_path)       */
  int32_t lane_bases;       /* bases per lane of the active path's kernel                                      */
  int32_t layout_build_us;  /* device time (HIP events, microseconds) batch_create spent building the direct layout -- the 16-byte records
                               and the payload runs -- from the caller's arrays; 0 for a batch over resident records (the decoder wrote it) */
  int64_t direct_general_reads;   /* reads that are not one or two gap-free match runs (walked op by op)      */
  int64_t direct_reach;           /* longest reference span of a read: how far back a tile's read range reaches */
  int64_t direct_stream_reads;    /* sum over tiles of the reads their streams hold: n_reads + straddlers when sorted */
  int64_t direct_max_tile_reads;
  int32_t direct_chunk_tiles;     /* the direct path's work items: chunks of this many consecutive tiles, a read visited once per chunk and a
                                     tile's overhang carried on (4), or 1: every tile by itself (unsorted positions, reads longer than the
                                     longest overhang, more outlier reads than their list holds)                                              */
  int32_t direct_overhang;        /* sites behind a tile's last that its tallies hold: 160, or 288 for a batch whose longest read asks for it */
} midas_snps_batch_info;
int32_t midas_snps_batch_get_info(const midas_snps_batch* batch, midas_snps_batch_info* out);
/* Device-side durations from HIP events recorded on the run's stream.  enable_timing(batch, n_slots)
 * allocates n_slots event triples (0 = off); run number k (counted from enable) records into slot
 * k % n_slots, so a caller can time K asynchronous runs and read all K after one sync.
 * out_ms: [0] index kernel (+ workspace memsets), [1] pileup kernel, [2] whole run.
 * time_pileup_only(batch, 1): runs record only the two events around the pileup kernel (each event record takes
 * ~4 us of stream time); out_ms[0] is then 0 and out_ms[2] == out_ms[1].                              */
int32_t midas_snps_batch_enable_timing(midas_snps_batch* batch, int32_t n_slots);
int32_t midas_snps_batch_time_pileup_only(midas_snps_batch* batch, int32_t on);
int32_t midas_snps_batch_timing(midas_snps_batch* batch, int32_t slot, float out_ms[3]);
/* Enqueue (same stream) a device-to-device copy of the per-species counters [n_species*4] i64 of the
 * last run into caller-owned device memory -- e.g. a torch tensor that is then all-gathered over
 * RCCL; the counters never round-trip through the host.  Replaces the pickled (species_id, aln_stats)
 * tuples returned through the Pool pipe (midas/run/snps.py:216, 228).                             */
int32_t midas_snps_batch_stats_to_device(midas_snps_batch* batch, void* dst_device_i64);

/* ---- host I/O (no GPU needed) ------------------------------------------------
 * BAM decode.  Replaces `pysam.AlignmentFile(bampath, 'rb')` and htslib's record decode
 * (midas/run/snps.py:186): the whole coordinate-sorted snps/temp/genomes.bam is inflated (BGZF blocks in
 * parallel) and every record with refID >= 0 -- everything fetch(contig, 0, length) can return -- is
 * decoded into the BAM-native SoA of midas_snps_reads plus a refID per record.  No .bai is needed
 * (index_bam, midas/run/snps.py:130-137, becomes a no-op: the device indexes).                     */
typedef struct midas_bam midas_bam;
int32_t midas_bam_open(const char* path, midas_bam** out, char* err256);
void midas_bam_close(midas_bam* bam);
int32_t midas_bam_n_refs(const midas_bam* bam);
int32_t midas_bam_ref(const midas_bam* bam, int32_t i, const char** name, int64_t* length);
/* Decode; returns the array sizes the caller must allocate for midas_bam_copy(). */
int32_t midas_bam_load(midas_bam* bam, int64_t* n_reads, int64_t* seq_bytes, int64_t* qual_bytes,
                       int64_t* n_cigar, char* err256);
/* The decoded columns where they are, without a copy: out12 = {refid, pos, mapq, flag, nm, l_seq, seq_off, qual_off,
 * cigar_off, seq4, qual, cigar} (types as in midas_bam_copy).  They belong to `bam` and are valid until midas_bam_close:
 * the caller keeps the handle for as long as it uses them (the Python host wraps them as numpy arrays that do).      */
int32_t midas_bam_columns(const midas_bam* bam, const void** out12);
/* Copy the decoded arrays out (any pointer may be NULL); *_off arrays have n_reads+1 entries. */
int32_t midas_bam_copy(const midas_bam* bam, int32_t* refid, int32_t* pos, uint8_t* mapq, uint16_t* flag,
                       int32_t* nm, int32_t* l_seq, int64_t* seq_off, int64_t* qual_off, int64_t* cigar_off,
                       uint8_t* seq4, uint8_t* qual, uint32_t* cigar);

/* Rank-local decode (N GPUs, one process each): a rank must not inflate the whole BAM to use an eighth of it.
 *   midas_bam_open_slice   maps the file, reads the BGZF block table and the header, and walks the records that START in
 *                          this rank's share of the file's bytes (slice of n_slices).  A slice that does not begin at
 *                          the header's end has to GUESS its first record boundary (32 plausible records in a row);
 *   midas_bam_slice_facts  hands back what the walk found -- out7 = {first record offset, offset behind the slice's last
 *                          record, coordinate-sorted so far (0/1), first and last refID seen, offset of the file's first
 *                          record, uncompressed size}; per reference: records, sum(l_seq), offset of its first record
 *                          (-1 = none in this slice).  All offsets are into the uncompressed stream.  The caller
 *                          exchanges these few numbers between the ranks and TRUSTS a guessed start only when the slice
 *                          before it ended on exactly that offset (the chain starts at the header's end, which is
 *                          exact): guesses are verified, never believed;
 *   midas_bam_load_ranges  inflates only the blocks that hold the given record ranges [begin, end) (e.g. the contigs
 *                          this rank owns: from a reference's first record to the next reference's) and decodes them;
 *                          midas_bam_copy then hands the columns out as after midas_bam_load.
 * Replaces the same `pysam.AlignmentFile` + `fetch(contig, ...)` of midas/run/snps.py:186, 194-199 (which goes through
 * the .bai the reference builds at :130-137; no index file is needed here).                                           */
int32_t midas_bam_open_slice(const char* path, int32_t slice, int32_t n_slices, midas_bam** out, char* err256);
/* The ONE-PASS form of the rank-local decode, for a coordinate-sorted BAM whose references are short beside a rank's share
 * (the usual metagenome: thousands of contigs): the file is dealt to the ranks as CONTIGUOUS runs of whole references.  Rank
 * `slice` of `n_slices` looks where its equal share of the file's bytes begins, guesses a record start there and walks the
 * records -- on the host, a few blocks -- to the first record of the next reference, at most max_walk uncompressed bytes on.
 * out3 = {first, total, rec_begin}: `first` = the uncompressed offset its share begins at (rec_begin for slice 0; `total` for an
 * empty share; -1: no reference border within max_walk -- a long chromosome: plan with midas_bam_open_slice instead).  The ranks
 * exchange their `first` (one all-gather of one number each) and every rank decodes [first of its own, first of the next) ONCE
 * with midas_bam_load_ranges / _device on this handle -- which also proves the next rank's guess: a range must end exactly on a
 * record border, and rank 0 starts at the header's end.  The reference reads the file once per worker through the index
 * (midas/run/snps.py:186-199); so does this, without an index.                                                          */
int32_t midas_bam_open_share(const char* path, int32_t slice, int32_t n_slices, int64_t max_walk, midas_bam** out, int64_t* out3,
                             char* err256);
/* The decoder's inverse (host only; what puts the synthetic samples of bench.py and the tests on disk -- samtools is not in
 * the image): records in the given order, refid[i] = reference of record i (-1: unmapped), names "r<i>", aux = NM + YT:Z:UU,
 * BGZF blocks of 0xff00 bytes deflated at `level` (0-9) by `threads` threads (0: the CPU budget), CRC-32 and the EOF block
 * as the specification wants them.  No reference counterpart (bowtie2 | samtools view | samtools sort write genomes.bam,
 * midas/run/snps.py:97-128).                                                                                         */
int32_t midas_bam_write(const char* path, int32_t n_ref, const char* const* ref_names, const int64_t* ref_lens,
                        const midas_snps_reads* reads, const int32_t* refid, int32_t level, int32_t threads, char* err256);
/* The same decoders with the BGZF blocks inflated ON THE DEVICE of `ctx` (bgzf_inflate.hip: one lane per block decodes its
 * Huffman codes -- by comparison against per-length limits in registers -- into tokens, a wavefront per block lays the bytes out) instead of by the host's threads: the compressed bytes go up, the inflated stream comes back, records are
 * walked and decoded into columns by the host as before.  On a 16-CPU host inflating is two thirds of the pileup stage once
 * the pileup and the row coder are on the device; with eight ranks sharing a node's CPUs it is more.  Same results, same
 * statuses (a corrupt block: MIDAS_SNPS_ERR_BAD_LAYOUT).  At this boundary a device failure is a status (ERR_OUT_OF_MEMORY,
 * ERR_HIP), never a silent fall-back; the Python host (midas_amd/run/snps.py, --device_inflate auto) answers those two with the
 * host decode and passes every other status on.
 *   midas_bam_open_device          = midas_bam_open (whole file; then midas_bam_load as usual)
 *   midas_bam_open_slice_device    = midas_bam_open_slice with the slice's blocks inflated AND walked on the device (bam_walk.hip):
 *                                  what comes down is refID / pos / l_seq / reference span / offset of the slice's records, which
 *                                  the host folds into the same facts (a rank of an 8-rank node has two CPUs for a gigabyte of BAM)
 *   midas_bam_load_ranges_device   = midas_bam_load_ranges on a handle of midas_bam_open_slice, decoded like midas_bam_load_device:
 *                                  SEQ / QUAL / CIGAR of the ranges' records stay on the device (midas_bam_payload_on_device == 1)
 *   midas_snps_inflate_blocks      the inflater on its own: n raw DEFLATE streams comp[cpos[k], +clen[k]) -> out[upos[k],
 *                                  +ulen[k]) (host pointers; every stream must inflate to exactly ulen[k] bytes and, when
 *                                  `crc` is not NULL, to bytes whose CRC-32 is crc[k]).  On a corrupt stream *bad_block (may
 *                                  be NULL) is its index.
 * Every BGZF block is held to the CRC-32 in its footer on both decoders, as htslib's bgzf_read_block does: a block that
 * inflates to the right size from damaged bytes is MIDAS_SNPS_ERR_BAD_LAYOUT naming the block's file offset.
 * Replaces the inflate inside pysam.AlignmentFile / htslib's bgzf.c behind midas/run/snps.py:186.
 *   midas_bam_load_device          open + load in one call, and SEQ / QUAL / CIGAR never come down: the host walks the
 *                                  records and decodes the small columns from the inflated stream as before, the three payload
 *                                  columns are cut out of the stream where it lies on the device.  midas_bam_columns then hands
 *                                  out DEVICE addresses for entries 9-11 (midas_bam_payload_on_device says so; midas_bam_copy
 *                                  refuses them), which midas_snps_batch_create / midas_snps_pileup accept in
 *                                  midas_snps_reads.seq4 / qual / cigar (they copy device to device).  They belong to `bam`.
 *   midas_snps_copy_from_device    bytes of such a column into host memory (tests; host code that must slice a payload).   */
int32_t midas_bam_open_device(const char* path, midas_snps_ctx* ctx, midas_bam** out, char* err256);
int32_t midas_bam_open_slice_device(const char* path, int32_t slice, int32_t n_slices, midas_snps_ctx* ctx, midas_bam** out, char* err256);
int32_t midas_bam_load_device(const char* path, midas_snps_ctx* ctx, midas_bam** out, int64_t* n_reads, int64_t* seq_bytes,
                              int64_t* qual_bytes, int64_t* n_cigar, char* err256);
int32_t midas_bam_payload_on_device(const midas_bam* bam);
/* The aligner's SAM TEXT instead of a BAM, parsed and coordinate-sorted on the device of `ctx` (sam_scan.hip).  bowtie2 writes SAM;
 * the reference pipes it through `samtools view -b | samtools sort` into snps/temp/genomes.bam (midas/run/snps.py:116-120) and opens
 * that (:186).  This call replaces the three: the file is mapped, its '@' lines are read by the host (@SQ SN: / LN: give the
 * references in file order; every other header line is skipped), the record lines go up in chunks that end on a complete line
 * (bounded by the free device memory; MIDAS_SNPS_SAM_CHUNK_BYTES, read at every call, overrides the size -- the decoded bytes do
 * not depend on it), one thread a line decodes FLAG, RNAME -> refID, POS (0-based; POS 0 -> -1), MAPQ, l_seq, the CIGAR's op
 * count and the first NM:i: tag (-1: none), a wave a line turns SEQ into 4-bit codes ("=ACMGRSVTWYHKDBN", either case, anything
 * else 15), QUAL into phred bytes ('*': l_seq bytes of 0xFF) and the CIGAR text into len << 4 | op words, and the records with
 * a reference (RNAME '*' is dropped, as the BAM decode drops refID < 0) are sorted by (refID, pos + 1) with the library's stable
 * radix sort -- equal keys keep file order.  The handle then answers midas_bam_n_refs / _ref / _columns / _payload_on_device /
 * _close exactly as one of midas_bam_load_device does: small columns in host memory, entries 9-11 of midas_bam_columns device
 * addresses, midas_bam_copy refuses them.  QNAME, RNEXT, PNEXT, TLEN and every tag but NM are not stored.
 * MIDAS_SNPS_ERR_BAD_LAYOUT, the message naming the 1-based line of the file (the first bad line in file order): an @SQ without
 * SN: or LN:, a repeated SN:, a record in front of any @SQ; a line of fewer than 11 fields; FLAG / POS / MAPQ that are not
 * decimal or beyond 65535 / 2^31 - 1 / 255; an RNAME that no @SQ names; a CIGAR op outside MIDNSHP=X, without a length, with
 * one of 2^28 or more, or more than 65535 ops; a QUAL that is not '*' and has not l_seq characters in '!'..'~'; an NM:i: whose
 * value is no integer.  MIDAS_SNPS_ERR_UNSUPPORTED: more than 2 * 10^9 records, 4 GiB of QUAL or 2^32 CIGAR ops in one file
 * (the sorted offsets are rebuilt by the library's 32-bit scan), a line longer than 1 GiB.  No host decoder stands behind it.
 *   midas_sam_decode_timing   host-clock milliseconds of the context's last midas_sam_load_device: out_ms8 = {map + header, upload,
 *                             line index, pass 1 (fields), scans, pass 2 (payload), sort + gather, columns down}
 *                             (measurement aid; no reference counterpart).                                                  */
int32_t midas_sam_load_device(const char* path, midas_snps_ctx* ctx, midas_bam** out, int64_t* n_reads, int64_t* seq_bytes,
                              int64_t* qual_bytes, int64_t* n_cigar, char* err256);
int32_t midas_sam_decode_timing(const midas_snps_ctx* ctx, float* out_ms8);
/* The same decode with the order of the records chosen by the caller.  MIDAS_SAM_ORDER_COORDINATE: midas_sam_load_device, to the
 * byte.  MIDAS_SAM_ORDER_FILE: the records that have a reference in the order of their lines -- what `samtools view -b` of the
 * aligner's output holds, and the order midas_genes_count's fp64 sums follow (run_midas.py genes --sam).  Nothing is sorted and
 * nothing is gathered: the columns the chunk loop accumulated are the result (64 zero bytes behind each payload column, as in
 * the sorted form), so the limits of 4 GiB of QUAL / 2^32 CIGAR ops do not apply and slot "sort + gather" of
 * midas_sam_decode_timing stays 0.  Every field rule, message and status is midas_sam_load_device's; another `order` is
 * MIDAS_SNPS_ERR_INVALID_ARG.                                                                                                 */
#define MIDAS_SAM_ORDER_COORDINATE 0
#define MIDAS_SAM_ORDER_FILE 1
int32_t midas_sam_load_device_order(const char* path, midas_snps_ctx* ctx, int32_t order, midas_bam** out, int64_t* n_reads,
                                    int64_t* seq_bytes, int64_t* qual_bytes, int64_t* n_cigar, char* err256);
/* The SAM decode straight into the pileup kernel's own layout: what midas_bam_load_resident (below) is to midas_bam_load_device.
 * The chunk loop, both passes and the coordinate sort are midas_sam_load_device's; the gather behind the sort writes every sorted
 * record ONCE, as its 16-byte record and its [cigar][quality sum][one byte a base] payload run, straight from the columns pass 2
 * accumulated in file order -- no sorted SEQ / QUAL / CIGAR column is built, the small columns and the offsets stay on the device,
 * and only refID comes down.  The handle is in the state a streamed midas_bam_load_resident leaves: midas_bam_is_resident 1,
 * midas_bam_columns entry 0 (refID, host) and NULL elsewhere, midas_bam_n_refs / _ref / _close as before,
 * midas_snps_batch_create_resident and midas_bam_resident_to_columns take it unchanged (raw columns, when asked for, are cut out of
 * the direct layout; the reads its bytes cannot give back exactly -- an IUPAC letter or '=', an A/C/G/T quality above 50, another
 * base's above 51, QUAL '*' -- lie raw in a side buffer that pass 2's flags size exactly before the gather is launched).
 * *sum_l_seq: the bases of all records.  Every field rule, message and status is midas_sam_load_device's (the first bad line in
 * file order, 1-based), and so are its limits; besides, MIDAS_SNPS_ERR_UNSUPPORTED: more than 32 GiB of read payload (the
 * record's offset is 32 bits of 8-byte units) -- decode with midas_sam_load_device instead.  midas_sam_decode_timing keeps its
 * eight slots: "sort + gather" covers the new gather, "columns down" is refID alone.                                            */
int32_t midas_sam_load_resident(const char* path, midas_snps_ctx* ctx, midas_bam** out, int64_t* n_reads, int64_t* sum_l_seq, char* err256);
/* A handle of midas_bam_open_slice / _open_share whose ranges are loaded needs its file no more: the mapping is handed to a
 * thread that unmaps it (a page-table walk of 0.2 s for a 9 GB BAM) while the caller piles the records up; the columns / the
 * resident records stay.  midas_bam_load_ranges* on the handle afterwards is MIDAS_SNPS_ERR_INVALID_ARG.                       */
void midas_bam_release_file(midas_bam* bam);
int32_t midas_snps_copy_from_device(midas_snps_ctx* ctx, void* dst, const void* src, int64_t bytes);
int32_t midas_bam_load_ranges_device(midas_bam* bam, midas_snps_ctx* ctx, int32_t n_ranges, const int64_t* range_begin,
                                     const int64_t* range_end, int64_t* n_reads, int64_t* seq_bytes, int64_t* qual_bytes,
                                     int64_t* n_cigar, char* err256);
/* ONE pass from the BAM's bytes to the pileup kernel's input (round 6).  The reference opens the BAM and counts in one go
 * (midas/run/snps.py:186-199); so does this: the decode above with NOTHING cut into columns and gathered back -- a record's CIGAR
 * ops, 4-bit SEQ and QUAL are one run of its bytes, in the order the direct path's payload has, and the device decoder copies that
 * run ONCE into the payload and writes the read's 16-byte record beside it.  Every column stays where the device decoded it
 * ("resident"); the host gets refID alone (midas_bam_columns: entry 0, the others NULL -- it groups the records by contig with it).
 *   midas_bam_load_resident          = midas_bam_load_device; *sum_l_seq: the bases of all records (what a caller sizes batches by)
 *   midas_bam_load_ranges_resident   = midas_bam_load_ranges_device
 *   midas_snps_batch_create_resident = midas_snps_batch_create over the handle's records [first_read, first_read +
 *                                      contigs->read_begin[n_contigs]) where they lie: nothing is uploaded, copied or built; the
 *                                      batch's facts pass validates them as it validates a caller's arrays.  The batch borrows the
 *                                      handle's device memory: midas_bam_close comes AFTER midas_snps_batch_destroy.  The packed and the
 *                                      long path (unsorted positions, coverage hot spots, reads beyond the fast paths' limits) cut
 *                                      their three payload columns out of the handle's inflated stream (or, after a streamed
 *                                      decode, out of the direct layout) when first asked for.
 *   midas_bam_resident_to_columns    the fall-back for a host that must regroup or slice the records (contigs it does not
 *                                      want among them, pieces of long contigs): the small columns come down, SEQ / QUAL /
 *                                      CIGAR are cut into device columns -- the handle then answers as after midas_bam_load_device
 *                                      (and stays resident as well).
 * A resident decode of ONE run of blocks that fills the device's decoder several times over (> ~51 000 BGZF blocks on MI355X: a BAM
 * of more than ~1.3 GB) is STREAMED: groups of blocks go up on a thread of their own while the groups before them are inflated,
 * walked and written behind one another into the resident layout; device memory is a few slots of ~2.5 x a group's inflated bytes
 * + the result instead of ~2.3 x the file's inflated bytes, and no inflated stream is kept.  Same records, same statuses (a corrupt
 * block is named by its index in the file).  Environment (read at every call): MIDAS_SNPS_DECODE_STREAM=0 switches it off,
 * MIDAS_SNPS_DECODE_GROUP_BLOCKS / _SLOTS (1-4) / _SLOT_MB size the groups, their number in flight and a slot's cap.
 * MIDAS_SNPS_ERR_UNSUPPORTED: more than 32 GiB of read payload in one decode (the record's offset is 32 bits of 8-byte units):
 * decode with midas_bam_load_device instead.                                                                                    */
int32_t midas_bam_load_resident(const char* path, midas_snps_ctx* ctx, midas_bam** out, int64_t* n_reads, int64_t* sum_l_seq, char* err256);
int32_t midas_bam_load_ranges_resident(midas_bam* bam, midas_snps_ctx* ctx, int32_t n_ranges, const int64_t* range_begin,
                                       const int64_t* range_end, int64_t* n_reads, int64_t* sum_l_seq, char* err256);
int32_t midas_bam_is_resident(const midas_bam* bam);
/* midas_bam_open_share with a LOCAL block table (round 6): a rank of N walks the BGZF chain over its own 1 / N of the file's bytes
 * only -- eight ranks that each walk, and page in the block headers of, the whole of a 9 GB file spend a third of a second each on
 * it.  _open_share_local: out4 = {file offset of the share's first block (a guess: a header from which eight headers follow one
 * another), where the rank's walk ended, uncompressed bytes of its blocks, file size}.  The ranks exchange these and believe them
 * only if they CHAIN (rank 0 starts at 0, every walk ends where the next begins, the last at the file's end); then
 * _share_locate(bam, slice, upos_base = the uncompressed bytes of the ranks in front, total = of all ranks, max_walk, out3) puts the
 * table in its place and finds the share's first record: out3 as midas_bam_open_share's.  midas_bam_load_ranges* walk the chain on
 * as far as a range reaches.  Ranks whose walks do not chain open their shares with midas_bam_open_share.                          */
int32_t midas_bam_open_share_local(const char* path, int32_t slice, int32_t n_slices, midas_bam** out, int64_t* out4, char* err256);
int32_t midas_bam_share_locate(midas_bam* bam, int32_t slice, int64_t upos_base, int64_t total, int64_t max_walk, int64_t* out3, char* err256);
int32_t midas_bam_resident_to_columns(midas_bam* bam, midas_snps_ctx* ctx, int64_t* seq_bytes, int64_t* qual_bytes, int64_t* n_cigar, char* err256);
int32_t midas_snps_batch_create_resident(midas_snps_ctx* ctx, const midas_snps_contigs* contigs, const midas_bam* bam, int64_t first_read,
                                         midas_snps_batch** out_batch);
int32_t midas_snps_inflate_blocks(midas_snps_ctx* ctx, const uint8_t* comp, int64_t comp_bytes, int64_t n_blocks,
                                  const int64_t* cpos, const int32_t* clen, const int64_t* upos, const int32_t* ulen,
                                  const uint32_t* crc, uint8_t* out, int64_t out_bytes, int64_t* bad_block);
int32_t midas_bam_slice_facts(const midas_bam* bam, int64_t* out7, int64_t* ref_reads, int64_t* ref_bases,
                              int64_t* ref_first);
/* What the walk of midas_bam_open_slice noted for cutting LONG references into pieces (midas_snps_contigs.origin), so that a
 * rank that owns a piece of a 20 Mb contig inflates that piece's records and not the contig's:
 *   out4     = {positions non-decreasing inside every reference so far (0/1), position of the slice's first and of its last
 *               mapped record (-1: none), number of marks};
 *   ref_span   [n_ref] the longest stretch of reference a record of that reference covers (M, D, N, =, X lengths summed): a
 *               piece that starts at `lo` needs the records from position lo - max-over-slices(ref_span) on;
 *   marks      [3 * n] {refID, bin, offset}: offset (uncompressed stream) of the first record of refID whose position is in
 *               [bin, bin + 1) * MIDAS_BAM_MARK_SPAN or, when that bin has none, in a later bin -- listed whenever the bin
 *               goes up, bin > 0 only (bin 0 is ref_first).  With positions sorted, every record of refID at a position >=
 *               bin * MIDAS_BAM_MARK_SPAN lies at or behind the smallest such offset over the slices.
 * marks may be NULL (ask for the count first); marks_capacity is in marks.                                               */
#define MIDAS_BAM_MARK_SPAN 65536
int32_t midas_bam_slice_marks(const midas_bam* bam, int64_t* out4, int64_t* ref_span, int64_t* marks, int64_t marks_capacity);
int32_t midas_bam_load_ranges(midas_bam* bam, int32_t n_ranges, const int64_t* range_begin, const int64_t* range_end,
                              int64_t* n_reads, int64_t* seq_bytes, int64_t* qual_bytes, int64_t* n_cigar, char* err256);

/* Row formatter + gzip writer for <outdir>/snps/output/<species>.snps.gz.  Replaces the per-site emit
 * loop of midas/run/snps.py:201-210 and utility.iopen(...,'w') (midas/utility.py:194-206) for ONE contig:
 * rows `ref_id \t i+1 \t allele[i] \t A+C+G+T \t A \t C \t G \t T \n` for i in [0, n_sites).
 * append == 0 creates the file and writes the header line first; append != 0 appends gzip members
 * (concatenated members are one valid gzip stream).  Rows are formatted and deflated by `threads`
 * workers (0 = all hardware threads) in 16 384-row members and written in order.  gz_level 1-5: the library's row
 * coder (midas_snps_deflate_rows below: smaller than zlib level 6 on these tables, several times faster);
 * 6-9: zlib at that level; 0: stored.                                                              */
int32_t midas_snps_write_rows(const char* path, int32_t append, const char* ref_id, int64_t n_sites,
                              const uint8_t* allele, const uint32_t* counts, int32_t gz_level,
                              int32_t threads, char* err256);
/* All contigs of one species in ONE call (header + rows, same text as repeated midas_snps_write_rows calls):
 * the emit loop of species_pileup over sorted(contigs) (midas/run/snps.py:183-213).  ref_ids[k], n_sites[k],
 * allele[k], counts[k] describe contig k in output order; the formatter/deflater pool works across contigs.  */
int32_t midas_snps_write_table(const char* path, int32_t n_contigs, const char* const* ref_ids,
                               const int64_t* n_sites, const uint8_t* const* allele, const uint32_t* const* counts,
                               int32_t gz_level, int32_t threads, char* err256);

/* A PART of a species' table: the rows of some of its contigs (consecutive in the sorted-contig order of the emit
 * loop), with or without the header member in front.  When a species' contigs are spread over several GPUs every
 * rank writes the parts it owns and the parts are concatenated in sorted-contig order: gzip members concatenate into
 * one valid gzip stream, and because a member never spans two contigs the concatenation is byte for byte the file
 * one midas_snps_write_table call would have written (midas/run/snps.py:183-213).                                */
int32_t midas_snps_write_part(const char* path, int32_t with_header, int32_t n_contigs, const char* const* ref_ids,
                              const int64_t* n_sites, const uint8_t* const* allele, const uint32_t* const* counts,
                              int32_t gz_level, int32_t threads, char* err256);
/* The same for entries that are PIECES of contigs (midas_snps_contigs.origin): entry k's first row is position
 * first_pos[k] + 1 of ref_ids[k] (first_pos NULL: all 0).  A piece's members are cut every MIDAS_SNPS_ROWS_PER_MEMBER rows
 * from its first row, so when every piece but a contig's last holds a multiple of that many rows the concatenated pieces
 * are byte for byte the rows of the whole contig.  (midas_snps_batch_write_part does this by itself from the origins the
 * batch was created with.)                                                                                          */
#define MIDAS_SNPS_ROWS_PER_MEMBER 16384
int32_t midas_snps_write_pieces(const char* path, int32_t with_header, int32_t n_contigs, const char* const* ref_ids,
                                const int64_t* n_sites, const int64_t* first_pos, const uint8_t* const* allele,
                                const uint32_t* const* counts, int32_t gz_level, int32_t threads, char* err256);

/* The count columns of SEVERAL samples' tables in one go: what the lock-step zip over the samples' files does in
 * build_temp_count_matrix (midas/merge/snps.py:236-271, one r[-4:] per sample and row).  _open reads all files (in
 * parallel) and walks their gzip members' headers; rows_each[t] is table t's row count, or -1 for a file that does not
 * announce it (written by the reference): such a table is read with midas_snps_table_open instead.  _read_counts fills
 * out_counts[t][4 * n_rows] with rows [row_begin, row_begin + n_rows) of every table t whose pointer is not NULL: every
 * gzip member of every table is one task of a single parallel region (inflate, then the last four fields of each line
 * straight into the caller's array) -- no per-table thread pools, no intermediate copies.                          */
typedef struct midas_snps_tableset midas_snps_tableset;
int32_t midas_snps_tableset_open(int32_t n_tables, const char* const* paths, midas_snps_tableset** out, int64_t* rows_each,
                                 char* err256);
int32_t midas_snps_tableset_read_counts(midas_snps_tableset* ts, int64_t row_begin, int64_t n_rows,
                                        uint32_t* const* out_counts, char* err256);
void midas_snps_tableset_close(midas_snps_tableset* ts);

/* The samples' count tables of one merge, RESIDENT on the device: n_samples x n_rows x 4 u32 (A, C, G, T), the layout the merge
 * kernels read.  _set_host uploads the first n_rows rows of one sample's table from a host array (a table the host read), _fetch
 * brings them down again (tests and tools), _shape says what the set was created with.  _free(NULL) is allowed.             */
typedef struct midas_merge_tables midas_merge_tables;
int32_t midas_merge_tables_create(midas_snps_ctx* ctx, int32_t n_samples, int64_t n_rows, midas_merge_tables** out);
void midas_merge_tables_free(midas_merge_tables* tables);
int32_t midas_merge_tables_shape(const midas_merge_tables* tables, int32_t* n_samples, int64_t* n_rows);
int32_t midas_merge_tables_set_host(midas_snps_ctx* ctx, midas_merge_tables* tables, int32_t sample, int64_t n_rows, const uint32_t* counts);
int32_t midas_merge_tables_fetch(midas_snps_ctx* ctx, const midas_merge_tables* tables, int32_t sample, int64_t n_rows, uint32_t* out);

/* midas_snps_tableset_read_counts on the device: for EVERY table t of the open set, rows [row_begin, row_begin + n_rows) -- n_rows
 * clipped to what the shortest table holds behind row_begin, as the host's zip over the files is -- end up in sample slot
 * first_sample_slot + t of `tables`, rows 0 ... .  The gzip members that hold those rows go up compressed, are inflated there
 * (every member's bytes checked against the CRC-32 and ISIZE of its trailer) and parsed there; nothing per row comes down.
 * Rows and values are accepted exactly as the host readers accept them (a row of more than 16 tabs included: fields 13-16, the
 * last one running to the end of the line).  Works in groups of members whose inflated text stays below a cap taken from the free
 * device memory (MIDAS_SNPS_MERGE_READ_KB overrides it; a member larger than the cap is a group by itself); a group's bytes go up
 * while the group before is in the kernels.  The result does not depend on the cap.
 * out_stats8 (nullable): tables, members read, groups, compressed bytes sent, inflated bytes, rows per table, groups with streams
 * decoded twice, 0.  out_ms4 (nullable): upload, inflate + CRC, line index, row parser (HIP events, summed over the groups).
 * A range that begins behind the shortest table's end is MIDAS_SNPS_ERR_INVALID_ARG, in midas_snps_tableset_read_counts' words.
 * MIDAS_SNPS_ERR_UNSUPPORTED: a file does not announce its rows (written by the reference): take midas_snps_tableset_read_counts /
 * midas_snps_table_open.  MIDAS_SNPS_ERR_BAD_LAYOUT, err256 naming the file: corrupt deflate data, a CRC-32 mismatch, a member that
 * holds another number of rows than it announces, or a malformed row (the lowest one of the table, as "malformed row N").
 * On any error nothing stays allocated; what `tables` holds in the slots is undefined then.                                  */
int32_t midas_snps_tableset_read_counts_device(midas_snps_ctx* ctx, midas_snps_tableset* ts, int64_t row_begin, int64_t n_rows,
                                               int32_t first_sample_slot, midas_merge_tables* tables, int64_t* out_stats8, float* out_ms4,
                                               char* err256);

/* The device's row parser on text of the caller's (tests: chosen rows reach the kernel without going through a file): the text
 * of ONE table of n_bytes (< 2^31), skip_header != 0: its first line is the header line.  *out_rows = rows found, the counts of
 * the first cap_rows of them in out_counts[4 * cap_rows]; *out_bad_row = the lowest malformed row among those (0-based), or -1.   */
int32_t midas_snps_parse_rows_device(midas_snps_ctx* ctx, const uint8_t* text, int64_t n_bytes, int32_t skip_header, uint32_t* out_counts,
                                     int64_t cap_rows, int64_t* out_rows, int64_t* out_bad_row);

/* The same rows as midas_snps_write_part, taken from a batch's results WHERE THEY ARE -- on the device -- for the
 * contigs contig_index[k] (indices into the batch's contig table, in output order) under the names ref_ids[k]: the
 * emit loop of species_pileup (midas/run/snps.py:183-213) without a host copy of the counts.  The formatter's
 * threads work on one slab of sites in the context's page-locked ring while the next slab crosses the link; the file
 * is byte for byte what batch_fetch + midas_snps_write_part write.  After midas_snps_batch_run.                  */
int32_t midas_snps_batch_write_part(midas_snps_batch* b, const char* path, int32_t with_header, int32_t n_contigs,
                                    const int32_t* contig_index, const char* const* ref_ids, int32_t gz_level,
                                    int32_t threads);

/* The row coder behind gz_level 1-5 of the writers above, on its own (tests and tools reach it here): a raw DEFLATE
 * stream (RFC 1951, one final dynamic-Huffman block) for text[0, n) whose rows start at row_begin[k] and whose row
 * tails -- the part that tends to repeat an earlier row: from the tab before ref_allele on -- start at tail_begin[k]
 * (row_begin[k] <= tail_begin[k] < row_begin[k + 1], the last row ends at n).  One table lookup per row instead of
 * zlib's hash chains: what utility.iopen's gzip.open(..., 'w') costs the reference (midas/utility.py:194-206,
 * midas/run/snps.py:179-210).  Any inflater reads the result.  Returns the stream's bytes in out[0, *out_len);
 * MIDAS_SNPS_ERR_INVALID_ARG when out_cap is too small (n + n/8 + 4096 always suffices).                          */
int32_t midas_snps_deflate_rows(const uint8_t* text, int64_t n, const uint32_t* row_begin, const uint32_t* tail_begin,
                                int64_t n_rows, uint8_t* out, int64_t out_cap, int64_t* out_len);

/* Parser of one sample's <species>.snps.gz: replaces read_run_midas_snps + the per-line split of
 * build_temp_count_matrix (midas/merge/snps.py:236-271): per row the site key '|'.join(r[0:3]) and the counts
 * r[-4:].  max_rows < 0 reads everything (args['max_sites']); want_keys == 0 skips the keys (only the first
 * sample's are used, as in the reference).  key_off has rows+1 entries into the key bytes.            */
typedef struct midas_snps_table midas_snps_table;
int32_t midas_snps_table_open(const char* path, int64_t max_rows, int32_t want_keys, midas_snps_table** out,
                              char* err256);
/* The same for the table rows [row_begin, row_end) only (row_end < 0: to the end) -- what one rank of a site-sharded
 * merge reads (the reference shards build_sharded_tables by line range, midas/merge/snps.py:366-386).  Tables written by
 * this library say in every gzip member how many rows it holds, so only the members that hold the range are inflated;
 * any other file is read whole and cut.  midas_snps_table_count_rows: the table's rows without inflating anything, or
 * -1 when the file does not say (a table written by the reference or by round 1 of this library).                    */
int32_t midas_snps_table_open_range(const char* path, int64_t row_begin, int64_t row_end, int32_t want_keys,
                                    midas_snps_table** out, char* err256);
int32_t midas_snps_table_count_rows(const char* path, int64_t* out_rows, char* err256);
void midas_snps_table_close(midas_snps_table* table);
int64_t midas_snps_table_rows(const midas_snps_table* table);
int64_t midas_snps_table_key_bytes(const midas_snps_table* table);
int32_t midas_snps_table_copy(const midas_snps_table* table, uint32_t* counts, char* keys, int64_t* key_off);

/* ---- merge_midas.py snps: per-site cross-sample arithmetic (SURVEY 8f "next" #1) -------------------
 * Replaces, for every genomic site of a species at once, GenomicSite.__init__/compute_pooled_counts,
 * call_alleles, compute_per_sample_mafs, compute_prevalence and flag
 * (midas/merge/snps.py:13-114, driven from build_sharded_tables :324-364).  Annotation (:116-174) and the
 * info line stay on the host; the rows of snps_freq.txt / snps_depth.txt (:196-201) are formatted on the device
 * by midas_merge_sites_tables, or on the host from midas_merge_sites' arrays (midas_merge_write_matrix).
 * Inputs are the samples' per-site count tables -- exactly what
 * the pileup stage emits -- and each sample's mean_coverage (midas/merge/merge.py:18-21).          */
typedef struct midas_merge_params {
  double allele_freq;   /* args['allele_freq']: freq >= allele_freq counts an allele as present (0.01)   */
  double site_ratio;    /* args['site_ratio']:  site_depth/mean_depth > site_ratio fails the sample (2.0) */
  double site_prev;     /* args['site_prev']:   prevalence < site_prev flags the site (0.95)              */
  int32_t site_depth;   /* args['site_depth']:  site_depth < site_depth fails the sample (1)              */
  int32_t snp_types;    /* args['snp_type'] as a bit set: 1 any, 2 mono, 4 bi, 8 tri, 16 quad             */
} midas_merge_params;
#define MIDAS_MERGE_ERR_ZERO_MEAN_DEPTH 7 /* ZeroDivisionError in compute_prevalence (snps.py:99) */
/* sample_counts[s] -> [n_sites*4] u32 (A,C,G,T per site) of sample s, host memory; mean_depth[s] = float(mean_coverage).
 * Outputs (host, caller-owned): calls [n_sites*4] = per site {major, minor, snp_type, flag}: major/minor 0..3 =
 * A,C,G,T, 255 = None; snp_type 0 None, 1 mono, 2 bi, 3 tri, 4 quad; flag 0 keep, 1 'min_prev', 2 'snp_type';
 * count_samples [n_sites], pooled [n_sites*4] u64, depth and minor_count [n_samples*n_sites] u32
 * (sample_depths and the numerator of sample_mafs; maf = float(minor_count)/depth if depth > 0 else 0.0).
 * out_kernel_ms (nullable): device time of the kernel(s), HIP events.                                */
int32_t midas_merge_sites(midas_snps_ctx* ctx, const midas_merge_params* params, int32_t n_samples, int64_t n_sites,
                          const uint32_t* const* sample_counts, const double* mean_depth, uint8_t* out_calls,
                          uint32_t* out_count_samples, uint64_t* out_pooled, uint32_t* out_depth, uint32_t* out_minor_count, float* out_kernel_ms);

/* snps_freq.txt / snps_depth.txt of merge_midas.py snps (GenomicSite.write, midas/merge/snps.py:196-201): header_line,
 * then one line per kept site `site_id \t v[sample 0] \t ...` with site_id = site_id_base + keep[r] + 1 (site_id_base: the
 * table row of the arrays' first site -- 0 unless the caller holds a row range of the table; header_line may be "").  depth / minor_count are
 * the [n_samples * n_sites] outputs of midas_merge_sites.  minor_count == NULL prints str(depth); otherwise
 * '{0:.3g}'.format(float(minor_count) / depth if depth > 0 else 0.0).  Host only, formatted by a thread pool.  */
int32_t midas_merge_write_matrix(const char* path, const char* header_line, int64_t n_keep, const int64_t* keep,
                                 int32_t n_samples, int64_t n_sites, const uint32_t* depth,
                                 const uint32_t* minor_count, int32_t threads, int64_t site_id_base, char* err256);

/* midas_merge_write_matrix with the rows formatted on the device: the host arrays go up, the text comes down through the
 * context's pinned ring and is written by one writer thread beside the formatting of the next batch.  Same arguments (no threads: there is no pool), the same
 * bytes in the file.  Written under a temporary name and renamed on success: an error leaves nothing at `path`.  Stricter
 * than the host writer where the device needs it: every keep[r] must lie in [0, n_sites), site_id_base >= 0, a minor count
 * above its (non-zero) depth is MIDAS_SNPS_ERR_INVALID_ARG, and kept rows out of ascending order are taken only while the
 * arrays fit one upload (MIDAS_SNPS_ERR_UNSUPPORTED otherwise).  The text is formatted in batches below a cap
 * (MIDAS_SNPS_MERGE_TEXT_MB, default 256; fractions allowed).  out_format_ms (nullable): device time of the formatter.   */
int32_t midas_merge_write_matrix_device(midas_snps_ctx* ctx, const char* path, const char* header_line, int64_t n_keep,
                                        const int64_t* keep, int32_t n_samples, int64_t n_sites, const uint32_t* depth,
                                        const uint32_t* minor_count, int64_t site_id_base, float* out_format_ms);

/* midas_merge_sites and both matrices in one call: depth and minor_count never come down -- per chunk of sites the kept
 * ones (flag == 0) are compacted on the device and the rows of snps_freq.txt (freq_path) and snps_depth.txt (depth_path)
 * formatted from the resident arrays; the text travels through the pinned ring while the next batch is formatted.  Both
 * files: header_line, then the rows, site_id = site_id_base + site + 1; written under temporary names and renamed on
 * success -- on any error neither exists.  out_calls / out_count_samples / out_pooled as midas_merge_sites;
 * *out_n_keep = rows written to each table; out_kernel_ms: the merge kernel alone; out_format_ms: compaction + formatter
 * (both nullable).  MIDAS_MERGE_ERR_ZERO_MEAN_DEPTH is reported as by midas_merge_sites.                                */
int32_t midas_merge_sites_tables(midas_snps_ctx* ctx, const midas_merge_params* params, int32_t n_samples, int64_t n_sites,
                                 const uint32_t* const* sample_counts, const double* mean_depth, const char* freq_path,
                                 const char* depth_path, const char* header_line, int64_t site_id_base, uint8_t* out_calls,
                                 uint32_t* out_count_samples, uint64_t* out_pooled, int64_t* out_n_keep, float* out_kernel_ms,
                                 float* out_format_ms);

/* The two calls above over a resident set (midas_merge_tables_*) in place of sample_counts: the samples are the set's, the sites
 * its first n_sites rows (n_sites <= the set's rows).  Everything else as above.  The host-array calls are these two behind a set
 * made from the arrays: the counts of all sites lie on the device at once, the per-site results are chunked as before.        */
int32_t midas_merge_sites_resident(midas_snps_ctx* ctx, const midas_merge_params* params, const midas_merge_tables* tables, int64_t n_sites,
                                   const double* mean_depth, uint8_t* out_calls, uint32_t* out_count_samples, uint64_t* out_pooled,
                                   uint32_t* out_depth, uint32_t* out_minor_count, float* out_kernel_ms);
int32_t midas_merge_sites_tables_resident(midas_snps_ctx* ctx, const midas_merge_params* params, const midas_merge_tables* tables, int64_t n_sites,
                                          const double* mean_depth, const char* freq_path, const char* depth_path, const char* header_line,
                                          int64_t site_id_base, uint8_t* out_calls, uint32_t* out_count_samples, uint64_t* out_pooled,
                                          int64_t* out_n_keep, float* out_kernel_ms, float* out_format_ms);

/* snps_info.txt of merge_midas.py snps: GenomicSite.annotate + fetch_ref_codon + the info line of GenomicSite.write
 * (midas/merge/snps.py:116-195) with utility.translate / index_replace (midas/utility.py:306-332) for the kept sites.
 * keys / key_off: 'ref_id|ref_pos|ref_allele' of every table row (midas_snps_table_copy); calls / count_samples /
 * pooled: outputs of midas_merge_sites; genes: the species' genes in the reference's order (scaffold_id, start, -end) --
 * scaffold ids, 1-based inclusive start/end, strand '+'/'-', gene_type and gene_id strings, and the gene sequence
 * oriented start to stop (get_gene_seq).  A site takes the first gene in that order that is not entirely behind it.  */
typedef struct midas_merge_genes {
  int64_t n_genes;
  const char* const* scaffold_id;
  const int64_t* start;
  const int64_t* end;
  const char* strand;          /* n_genes chars */
  const char* const* gene_type;
  const char* const* gene_id;
  const char* const* seq;
} midas_merge_genes;
int32_t midas_merge_write_info(const char* path, const char* header_line, int64_t n_keep, const int64_t* keep,
                               const char* keys, const int64_t* key_off, const uint8_t* calls,
                               const uint32_t* count_samples, const uint64_t* pooled, const midas_merge_genes* genes,
                               int32_t threads, int64_t site_id_base, char* err256);

/* ---- run_midas.py genes: reads per pangenome gene (SURVEY 8f "next" #4) -----------------------------------------
 * Replaces count_mapped_bp's pass over the BAM (midas/run/genes.py:165-180) for every gene at once: per gene the number
 * of alignments (aligned_reads), of alignments passing keep_read (genes.py:148-163 -- the same predicate as the snps
 * path, thresholds mapid / readq / mapq / aln_cov of `thr`; baseq unused) and depth = the sum, IN BAM ORDER, of
 * len(query_alignment_sequence) / float(gene_length) over the kept ones (fp64, bit-identical to the reference's
 * running sum).  reads: the alignments in BAM order (seq4 may be NULL: only l_seq, CIGAR, NM, QUAL and MAPQ are read);
 * ref_id[i]: index of read i's gene in gene_length.  A record the reference would raise on returns
 * MIDAS_SNPS_ERR_READ_NO_SEQ / _NO_NM / _ZERO_ALIGN / _NO_QUAL with the lowest offending read in
 * midas_snps_last_error_read.  out_kernel_ms (nullable): device time of the kernel.                                  */
int32_t midas_genes_count(midas_snps_ctx* ctx, const midas_snps_thresholds* thr, const midas_snps_reads* reads,
                          const int32_t* ref_id, int64_t n_genes, const int64_t* gene_length, int64_t* out_aligned,
                          int64_t* out_mapped, double* out_depth, float* out_kernel_ms);

/* midas_genes_count over reads whose QUAL and CIGAR columns lie on the context's DEVICE (reads->qual / ->cigar are device
 * addresses, as midas_snps_batch_create accepts them: a handle of midas_sam_load_device_order(MIDAS_SAM_ORDER_FILE), of
 * midas_bam_load_device or of midas_bam_load_ranges_device; reads->seq4 is not looked at).  The per-read pass over the
 * quality bytes and the CIGAR ends that midas_genes_count runs on the host's cores is a kernel here (genes_facts_kernel,
 * sixteen lanes a read); the small columns and ref_id are host memory and go up once (29 bytes a read).  reads->qual_off[n] /
 * ->cigar_off[n] are taken for the sizes of the two columns: nothing outside [qual, qual + qual_off[n]) and [cigar, cigar +
 * cigar_off[n]) is read, and a read whose offsets point outside them is MIDAS_SNPS_ERR_BAD_LAYOUT.  Everything behind the
 * records (filter, stable sort by gene, ordered sums) is shared with midas_genes_count:
 *   midas_genes_count_device(reads) == midas_genes_count(the same reads in host memory)
 * in every count, every depth bit for bit, the status and midas_snps_last_error_read (tests/test_gpu_genes_sam.py).
 *   midas_genes_count_timing   device milliseconds of the context's last midas_genes_count_device: out_ms2 = {facts kernel,
 *                              filter + sort + sums} (measurement aid; no reference counterpart).                         */
int32_t midas_genes_count_device(midas_snps_ctx* ctx, const midas_snps_thresholds* thr, const midas_snps_reads* reads,
                                 const int32_t* ref_id, int64_t n_genes, const int64_t* gene_length, int64_t* out_aligned,
                                 int64_t* out_mapped, double* out_depth, float* out_kernel_ms);
int32_t midas_genes_count_timing(const midas_snps_ctx* ctx, float* out_ms2);

/* midas_genes_count over genes/temp/pangenomes.bam itself, in ONE pass on the context's device: what midas_bam_load_resident is to
 * the snps path.  `bam`: an open handle on which nothing has been loaded (midas_bam_open_device, midas_bam_open, or -- cheapest, it
 * inflates the header's blocks only and keeps the file mapped with its block table -- midas_bam_open_share(path, 0, 1, 0, ...)); its
 * header is read, so the caller asks midas_bam_n_refs / midas_bam_ref first and hands gene_length[i] for reference i of the header.
 * n_genes must equal midas_bam_n_refs(bam) (else MIDAS_SNPS_ERR_INVALID_ARG).  The call leaves the handle as it was.
 * The steps are the device decode's own, in one arena: the file's BGZF blocks go up, are inflated and held to their CRC-32
 * (bgzf_inflate.hip), the records are walked in chunks and the chunks stitched (bam_walk.hip), every kept record's offset is
 * written -- and then, instead of columns, scans and a payload cut, bam_genes_facts_kernel (genes_count.hip) makes every read's
 * 8-byte fact from its record where it lies in the inflated stream: sixteen lanes a read sum its QUAL run, lane 0 walks the CIGAR
 * ends and finds NM in the aux block.  Filter, stable sort by gene, bounds and ordered fp64 sums are the tail midas_genes_count and
 * midas_genes_count_device run.  Nothing per read comes down: the three per-gene arrays do.
 *   midas_genes_count_bam(file) == midas_genes_count(midas_bam_open + midas_bam_load of the same file)
 * in every count, every depth bit for bit, and in the status; midas_snps_last_error_read agrees too -- it is the index among the
 * KEPT records (refID >= 0), as the host decode counts them (tests/test_gpu_genes_bam.py).
 * Statuses: the per-read ones of midas_genes_count; MIDAS_SNPS_ERR_BAD_LAYOUT for a corrupt BGZF block (err256 names its file
 * offset, as the other decoders do), a block_size that leaves the stream, a record whose variable parts overrun its block_size or
 * whose refID names no reference; MIDAS_SNPS_ERR_UNSUPPORTED for l_seq > 1024 or NM > 65534 (as midas_genes_count) and for
 * record boundaries the walk cannot settle; MIDAS_SNPS_ERR_OUT_OF_MEMORY for a file whose decode does not fit one arena (about
 * 2.3 x its inflated bytes; there is no streamed form); MIDAS_SNPS_ERR_HIP for a device failure -- a status, never a silent
 * fall-back (run_midas.py genes --device_inflate auto answers the last two with the host route).  err256 (nullable, 256 bytes)
 * and midas_snps_last_error hold the message.
 *   out_stats8 (nullable): records kept, records dropped for refID < 0, BGZF blocks, inflated bytes, chunks walked, chunks walked
 *                          again, 0, 0
 *   out_ms8 (nullable):    upload (host clock around a synchronise), then device events: inflate + CRC, walk + stitch + offsets,
 *                          facts kernel, filter + sort + sums, download, 0, 0 (measurement aid; no reference counterpart).     */
int32_t midas_genes_count_bam(midas_snps_ctx* ctx, midas_bam* bam, const midas_snps_thresholds* thr, int64_t n_genes,
                              const int64_t* gene_length, int64_t* out_aligned, int64_t* out_mapped, double* out_depth,
                              int64_t* out_stats8, float* out_ms8, char* err256);

/* The two halves of midas_genes_count, for N ranks below the species (midas_amd/run/genes.py): a gene's running fp64 sum has
 * to be formed in BAM order on ONE rank, so every rank turns ITS slice of the unsorted BAM into terms, the (gene, term) pairs
 * travel to the gene's owner (one all-to-all; the slices are in file order, so are the pairs a rank receives), and the owner sums.
 *   midas_genes_terms: out_term[i] = len(query_alignment_sequence) / float(gene_length[ref_id[i]]) for a read keep_read
 *     passes, +0.0 for one it drops (adding it leaves a running sum unchanged bit for bit: the pair still counts as an
 *     alignment of its gene).  Statuses and midas_snps_last_error_read as midas_genes_count (the read index is the slice's).
 *   midas_genes_sum: the pairs (gene[i] in [0, n_genes), term[i]), in the order their reads have in the BAM -> per gene
 *     the number of pairs (aligned_reads), of pairs with a term above zero (mapped_reads) and their sum in that order.
 * midas_genes_count(reads) == midas_genes_sum(ref_id, midas_genes_terms(reads)) bit for bit (tests/test_gpu_genes.py).     */
int32_t midas_genes_terms(midas_snps_ctx* ctx, const midas_snps_thresholds* thr, const midas_snps_reads* reads,
                          const int32_t* ref_id, int64_t n_genes, const int64_t* gene_length, double* out_term,
                          float* out_kernel_ms);
int32_t midas_genes_sum(midas_snps_ctx* ctx, int64_t n_pairs, const int32_t* gene, const double* term, int64_t n_genes,
                        int64_t* out_aligned, int64_t* out_mapped, double* out_depth, float* out_kernel_ms);

/* ---- merge_midas.py genes: cross-sample gene matrices ----------------------------------------------------------------------
 * Both readers parse as utility.parse_file does under Python 3 (midas/utility.py:208-216): universal newlines, '\t'-split
 * header and rows, a row whose field count differs from the header's skipped, a field taken from the LAST header column of
 * its name.  Numbers: float() / int() of the field, ASCII whitespace trimmed, plain decimal / nan / inf / infinity spellings
 * only (anything else is MIDAS_SNPS_ERR_BAD_LAYOUT naming file and line).  err1024 (nullable, 1024 bytes) receives the message.
 *
 * midas_genes_merge_map_*: read_cluster_map (midas/merge/genes.py:91-98) -- gene_info.txt[.gz] -> centroid_99 ->
 *   <cluster_column> (e.g. "centroid_95"), row by row, the last row of an id winning.  columns: out5[0..4] = the distinct
 *   clusters in sorted byte order back to back (char) and their offsets (int64, n_clusters + 1), the distinct centroid_99 ids
 *   in first-appearance order (char) and their offsets (int64, n_genes + 1), each id's cluster index (uint32, n_genes);
 *   sizes2 = bytes of the two id pools.  They belong to the handle.                                                         */
typedef struct midas_genes_merge_map midas_genes_merge_map;
int32_t midas_genes_merge_map_open(const char* path, const char* cluster_column, midas_genes_merge_map** out, char* err1024);
int64_t midas_genes_merge_map_n_clusters(const midas_genes_merge_map* m);
int64_t midas_genes_merge_map_n_genes(const midas_genes_merge_map* m);
int32_t midas_genes_merge_map_columns(const midas_genes_merge_map* m, const void** out5, int64_t* sizes2);
void midas_genes_merge_map_close(midas_genes_merge_map* m);

/* midas_genes_merge_tables_*: the per-sample parse of build_gene_matrices (midas/merge/genes.py:18-26) for n_tables
 *   genes.gz files, `threads` files at a time (0: all cores).  Per kept row: gene_id (ref_id when that column exists),
 *   copy_number (normalized_coverage when it exists) and coverage (raw_coverage) as f64, count_reads as i64 (0 without the
 *   column).  resolve: every row's gene id -> cluster index through the map (sp.map[...], genes.py:22; an id the map lacks is
 *   MIDAS_SNPS_ERR_BAD_LAYOUT); with reuse != 0 a table whose ids and offsets are byte-equal to an earlier table's takes
 *   that table's cluster vector (*out_same_as = its index, else -1).  columns: out6[0..5] = ids (char), id offsets (int64,
 *   rows + 1), copy (f64), depth (f64), reads (i64), clusters (uint32, after resolve).  They belong to the handle.         */
typedef struct midas_genes_merge_tables midas_genes_merge_tables;
int32_t midas_genes_merge_tables_open(int32_t n_tables, const char* const* paths, int32_t threads, midas_genes_merge_tables** out,
                                      char* err1024);
int64_t midas_genes_merge_tables_rows(const midas_genes_merge_tables* ts, int32_t table);
int32_t midas_genes_merge_tables_resolve(midas_genes_merge_tables* ts, const midas_genes_merge_map* m, int32_t reuse, int32_t threads,
                                         char* err1024);
int32_t midas_genes_merge_tables_columns(const midas_genes_merge_tables* ts, int32_t table, const void** out6, int64_t* out_id_bytes,
                                         int32_t* out_same_as);
void midas_genes_merge_tables_close(midas_genes_merge_tables* ts);

/* The arithmetic of build_gene_matrices (midas/merge/genes.py:12-30) on the device for n_samples tables of one species:
 * sample s has n_rows[s] rows with cluster[s][i] in [0, n_clusters) and copy / depth / reads columns (host memory).  Output
 * rows are the clusters sample 0's table mentions (sorted(sp.samples[0].genes['depth']), genes.py:40), in index order:
 * out_row_cluster[r]; per (row r, sample s) at r * n_samples + s: the fp64 sums of copy and depth over the sample's rows of
 * the cluster IN TABLE ORDER (starting from 0.0), the i64 sum of reads, and out_state = 0 (the cluster is not in the sample's
 * table: the defaultdict's 0.0 in presabs), 1 (present, copy < min_copy), 2 (present, copy >= min_copy).  out_capacity: rows
 * the outputs hold (min(n_clusters, n_rows[0]) always suffices); *out_n_rows: rows written.  group_samples: samples on the
 * device at a time (0: as many as a quarter of the free device memory holds); the bytes do not depend on it.
 * out_kernel_ms (nullable): device time of the kernels (sort, bounds, row list, transposes, merge), copies not counted.     */
int32_t midas_genes_merge(midas_snps_ctx* ctx, int32_t n_samples, const int64_t* n_rows, const uint32_t* const* cluster,
                          const double* const* copy, const double* const* depth, const int64_t* const* reads, int64_t n_clusters,
                          double min_copy, int32_t group_samples, int64_t out_capacity, int64_t* out_n_rows,
                          uint32_t* out_row_cluster, double* out_copy, double* out_depth, int64_t* out_reads, uint8_t* out_state,
                          float* out_kernel_ms);

/* genes_{presabs,copynum,depth,reads}.txt (write_gene_matrices, midas/merge/genes.py:32-48): header_line, then per row r
 * the cluster id of row_cluster[r] (ids / offsets as midas_genes_merge_map_columns gives them) and one cell per sample, str()
 * of the value.  kind 0 presabs: state 2 -> "1", 1 -> "0", 0 -> "0.0" (values unused); kind 1: values are f64, Python's repr;
 * kind 2: values are i64.  values / state: [n_rows * n_samples] as midas_genes_merge writes them.  Host only, row blocks
 * formatted by `threads` workers (0: all cores).
 * midas_genes_merge_format_f64: repr() of n doubles, each followed by '\n' (capacity >= 33 n bytes) -- the formatter alone. */
int32_t midas_genes_merge_write_matrix(const char* path, const char* header_line, int32_t kind, int64_t n_rows, const uint32_t* row_cluster,
                                       const char* cluster_ids, const int64_t* cluster_off, int32_t n_samples, const void* values,
                                       const uint8_t* state, int32_t threads, char* err1024);
int32_t midas_genes_merge_format_f64(int64_t n, const double* v, char* out, int64_t capacity, int64_t* out_len);

/* ---- snp_diversity.py / call_consensus.py: the analysis of one merged species directory ------------------------------------
 * midas_sites_tables_*: one output directory of `merge_midas.py snps`, read as csv.DictReader(delimiter='\t') reads it
 *   (midas/analyze/parse_snps.py:27-58, 181-194): snps_summary.txt and snps_info.txt parsed into columns, snps_freq.txt and
 *   snps_depth.txt mapped and left as text.  counts: out8[0..6] = summary rows, info rows, distinct gene ids, sample columns
 *   of the depth header, bytes of the freq and depth rows after their header lines, sample columns of the freq header.
 *   columns: out25[2k], out25[2k + 1] for k = 0..8 = the strings back to back (char) and their offsets (int64, n + 1) of
 *   sample_id, site_id, ref_allele, major_allele, minor_allele, locus_type, site_type, the gene ids in order of first
 *   appearance, the depth header's sample ids; sizes10[k] = bytes of pool k; out25[18..22] = mean_coverage (f64),
 *   fraction_covered (f64), the sites' gene index (int32, -1: no gene id), the freq rows, the depth rows (char).  They belong
 *   to the handle.  A file that cannot be read, or a row that lacks a field in use, is an error naming file and line.
 * midas_sites_parse_cell: float() (kind 0, out8 is a double) or int() (kind 1, an int64) of one cell by the host's exact
 *   parser -- the one the scan uses for the cells its device parser passes on.
 * midas_sites_tables_positions: the ref_id and ref_pos columns of the directory's snps_info.txt, read on the first call (the
 *   columns are found by the header's names; the rows are those of midas_sites_tables_columns).  out4 = the rows' contig index
 *   (int32, in order of first appearance of the ref_id), their ref_pos (int64, int() of the field), the contig names back to
 *   back (char) and their offsets (int64, n + 1); sizes2 = contigs, bytes of the names.  They belong to the handle.  A header
 *   without one of the two columns, a row without the field or a ref_pos that is no integer is an error naming file and line. */
typedef struct midas_sites_tables midas_sites_tables;
int32_t midas_sites_tables_open(const char* dir, midas_sites_tables** out, char* err1024);
int32_t midas_sites_tables_counts(const midas_sites_tables* t, int64_t* out8);
int32_t midas_sites_tables_columns(const midas_sites_tables* t, const void** out25, int64_t* sizes10);
int32_t midas_sites_tables_positions(midas_sites_tables* t, const void** out4, int64_t* sizes2, char* err1024);
void midas_sites_tables_close(midas_sites_tables* t);
int32_t midas_sites_parse_cell(int32_t kind, const char* text, int64_t n, void* out8);

/* The per-site loop of snp_diversity.py (:182-258) and call_consensus.py (:183-213) on the device.  freq / depth: the text
 * rows of the two matrices after their header lines (host memory); row i of both belongs to site i, and the sites end with
 * the shorter of the two or at n_sites_max.  Per site i: site_mask[i] (what the info table and the options decide: ref_allele,
 * locus / site type, --site_list, --rand_sites), site_gene[i] (MIDAS_SITES_PER_GENE), minor[i] / major[i] (MIDAS_SITES_SEQ).
 * Sample s of n_samples reads matrix column sample_col[s] (0 = the first after the site id) and has mean_depth[s]; the order
 * of the samples is the order of every sum over samples.  fparams5 = site_ratio, allele_support, site_prev, site_maf, snp_maf;
 * iparams8 = site_depth, max_sites (-1: all), flags, number of genes, group_rows, chunk_bytes (0: from the free device
 * memory; the outputs do not depend on either), sequence capacity, 0.
 * A cell is float() / int() of its text; the device converts plain decimals itself and hands every other cell to the host's
 * exact parser.  A row with too few columns or a cell that is no number, among the rows the reference would read, is
 * MIDAS_SNPS_ERR_BAD_LAYOUT with out_stats16[4..6] = matrix (1 freq, 2 depth), 0-based data row, sample (-1: short row).
 * So is a site whose pooled frequency the reference cannot form: [4] = 3, a frequency that is not finite under
 * MIDAS_SITES_ROUND (round() raises; [6] the first such sample, kept or not), or [4] = 6, kept samples whose depths sum to 0
 * under MIDAS_SITES_WEIGHT (a division by zero; [6] = -1).  The earliest row in file order is reported, a row's cells before
 * its site, and no site behind the row that fills max_sites (the one row the reference still reads has its cells checked,
 * whichever row group it falls in; max_sites 0 reads the first row's cells and nothing else).
 * MIDAS_SITES_SUMS: per chain (sample s, or the pool under MIDAS_SITES_POOLED) and gene (MIDAS_SITES_PER_GENE; else one) at
 *   chain * genes + gene: out_pi = the sum of 2 f (1 - f) in site order exactly as `+=` forms it, out_snps, out_sites,
 *   out_depth.  MIDAS_SITES_SEQ: out_seq[s * capacity + k] = '-', minor or major allele of the k-th retained site.
 * dump_* (nullable, tests): the parsed cells [n_samples][n_sites_max], the sites' final keep flag and pooled frequency.
 * out_stats16: [0] sites read, [1] sites kept, [2] / [3] freq / depth cells converted by the host, [7] row groups, [8] kept
 * sites without a gene under MIDAS_SITES_PER_GENE, [9] group_rows and [10] chunk_bytes in use.  out_ms8 (nullable): upload +
 * index (host clock), index, parse, site, order, sums, sequences, download (device events).
 * A matrix column selected twice in sample_col is MIDAS_SNPS_ERR_INVALID_ARG here and below, with n_sites_max 0 too.       */
#define MIDAS_SITES_WEIGHT 1
#define MIDAS_SITES_ROUND 2
#define MIDAS_SITES_POOLED 4
#define MIDAS_SITES_PER_GENE 8
#define MIDAS_SITES_MASK_ONLY 16
#define MIDAS_SITES_SEQ 32
#define MIDAS_SITES_SUMS 64
int32_t midas_sites_scan(midas_snps_ctx* ctx, const char* freq, int64_t freq_bytes, const char* depth, int64_t depth_bytes,
                         int64_t n_sites_max, const uint8_t* site_mask, const int32_t* site_gene, const char* minor, const char* major,
                         int32_t n_samples, const int32_t* sample_col, const double* mean_depth, const double* fparams5,
                         const int64_t* iparams8, double* out_pi, int64_t* out_snps, int64_t* out_sites, int64_t* out_depth,
                         uint8_t* out_seq, double* dump_freq, int64_t* dump_depth, uint8_t* dump_keep, double* dump_pooled,
                         int64_t* out_stats16, float* out_ms8);

/* midas_sites_scan with snp_diversity.py's --rand_reads N [--replace_reads] (GenomicSite.resample_reads): the arguments of
 * midas_sites_scan, then rand_reads = N (1 .. 2^31 - 1), replace, numpy's global legacy generator as np.random.get_state() gives
 * it (mt_key 624 words, mt_pos 0 .. 624), the state the reference's loop would leave it in (mt_key_out, mt_pos_out; they may be
 * mt_key's memory) and out_draw8 (nullable).  iparams8[7]: the most raw words one launch of the generator makes (0: chosen; the
 * outputs and the returned state depend neither on it nor on group_rows).  MIDAS_SITES_SEQ is MIDAS_SNPS_ERR_INVALID_ARG:
 * call_consensus.py has no such option.
 * A site is resampled when it is retained (max_sites counted) and its pooled frequency is > 0.  There every sample, kept or
 * not, gets depth N, and a cell with 0 < f < 1 (after rounding under MIDAS_SITES_ROUND: none) gets f = k / N with
 * count_minor = round(f * N), half to even, and k = count_minor without replacement, or with replacement the number of the
 * cell's N draws below count_minor.  The draws are np.random.randint(0, N, N)'s: 32-bit MT19937 words ANDed with the smallest
 * 2^j - 1 >= N - 1, those <= N - 1 accepted; the c-th cell that draws, sites in file order and samples in theirs, takes accepted
 * words [c N, (c + 1) N).  N = 1 draws nothing.  The site's pooled frequency is then formed again over the same kept samples,
 * and the sums see the new cells.  The state returned stands right behind the last accepted word used (rejected words before it
 * are consumed, none after it); without replacement, with N = 1 or when no cell draws it is the state given.
 * dump_*: the cells and pooled frequencies after resampling.  out_stats16 as midas_sites_scan, and [11] sites resampled,
 * [12] cells with 0 < f < 1 among them (the cells that draw, with replacement and N > 1).  out_draw8: [0] raw words generated,
 * [1] accepted words used, [2] raw words consumed (to the returned state), then ms of [3] eligibility, [4] generation,
 * [5] compaction, [6] resampling, [7] the pooled frequencies (device events; midas_sites_scan's out_ms8 holds the rest).       */
int32_t midas_sites_scan_resampled(midas_snps_ctx* ctx, const char* freq, int64_t freq_bytes, const char* depth, int64_t depth_bytes,
                                   int64_t n_sites_max, const uint8_t* site_mask, const int32_t* site_gene, const char* minor,
                                   const char* major, int32_t n_samples, const int32_t* sample_col, const double* mean_depth,
                                   const double* fparams5, const int64_t* iparams8, double* out_pi, int64_t* out_snps, int64_t* out_sites,
                                   int64_t* out_depth, uint8_t* out_seq, double* dump_freq, int64_t* dump_depth, uint8_t* dump_keep,
                                   double* dump_pooled, int64_t* out_stats16, float* out_ms8, int64_t rand_reads, int32_t replace,
                                   const uint32_t* mt_key, int32_t mt_pos, uint32_t* mt_key_out, int32_t* mt_pos_out, double* out_draw8);

/* midas_sites_scan's sums once per site class, in one pass over the rows (snp_pnps.py: class 0 the 1D sites, class 1 the 4D
 * sites): the arguments of midas_sites_scan, then site_class[i] = the class of site i and n_classes (1 .. 4).  With n_classes 1
 * site_class may be NULL: every site is class 0.  A site with site_mask on and a class >= n_classes is
 * MIDAS_SNPS_ERR_INVALID_ARG before anything runs; so is MIDAS_SITES_SEQ.  The class belongs to the sums alone: the rows, the
 * cells, the site decisions, max_sites (retained sites of all classes together), the dumps and out_stats16 are midas_sites_scan's
 * for the same site_mask, [8] included (a kept site without a gene counts once, whatever its class).
 * out_pi / out_snps / out_sites / out_depth are [n_classes][chains][genes]: block c is what midas_sites_scan writes for the
 * mask site_mask[i] && site_class[i] == c with the same retained sites -- pi the sequential sum in site order, bit for bit.       */
#define MIDAS_SITES_MAX_CLASSES 4
int32_t midas_sites_scan_classes(midas_snps_ctx* ctx, const char* freq, int64_t freq_bytes, const char* depth, int64_t depth_bytes,
                                 int64_t n_sites_max, const uint8_t* site_mask, const int32_t* site_gene, const char* minor,
                                 const char* major, int32_t n_samples, const int32_t* sample_col, const double* mean_depth,
                                 const double* fparams5, const int64_t* iparams8, double* out_pi, int64_t* out_snps, int64_t* out_sites,
                                 int64_t* out_depth, uint8_t* out_seq, double* dump_freq, int64_t* dump_depth, uint8_t* dump_keep,
                                 double* dump_pooled, int64_t* out_stats16, float* out_ms8, const uint8_t* site_class,
                                 int32_t n_classes);

/* ---- strain_tracking.py: marker alleles (id_markers) and their sharing between all pairs of samples (track_markers) ----------
 * Both walk the two matrices as midas_sites_scan does (same text, same cell parsers, same row groups, same place of a bad row
 * in out_stats16[4..6]).  Rows [0, n_parse) are read and checked, rows [0, n_call) are called (n_call <= n_parse: the reference
 * reads one row more than --max_sites lets it use).  An allele with frequency x (freq for the minor, 1 - freq for the major
 * allele) is present in a sample of depth d != 0 when x >= min_freq and round(x * d) >= min_reads, round() half to even.
 * fparams2 = min_freq, 0; iparams8 = min_reads, allele_prev, group_rows, chunk_bytes, capacity (markers), pair_blocks
 * (track_markers: the workgroups the pair kernel aims at when it cuts the words into runs; 0: 1024; the output does not
 * depend on it), 0, 0.
 * id_markers: minor_code / major_code [n_call]: 0..3 = the site's allele is A, T, C, G, anything else another string.  A site
 *   is a marker when exactly two letters are present in some sample and the rarer (a tie: the earlier of A, T, C, G) is present
 *   in at most allele_prev samples.  out_rows7 [capacity][7], in site order: site row, allele 0..3, samples with depth != 0,
 *   samples with A, T, C, G.  out_stats16[1] = markers.
 * track_markers: site_which [n_call]: 0 the site is no marker, 1 the marker is its major, 2 its minor allele.  The matched
 *   sites of a row group become a bit matrix [sample][64 sites a word]; out_both [n_samples][n_samples], filled for i <= j:
 *   sites whose marker is present in samples i and j (the diagonal: in sample i).  The sums are integers held on the device
 *   across row groups: they do not depend on group_rows.  A workgroup adds up a MIDAS_SITES_PAIR_TILE-square tile of pairs.
 *   out_stats16[1] = matched sites, [8] = (sample pairs with i <= j) x words of the bit matrices, [11] / [12] = the most word
 *   runs a launch of the pair kernel had and the most staging steps a run had.
 * A site that cannot be called is MIDAS_SNPS_ERR_BAD_LAYOUT with out_stats16[4] = 3 (frequency x depth is not finite), 4 / 5
 * (a sample has the minor / major allele, which is none of A, T, C, G), [5] the data row, [6] the sample.  Of a row that
 * cannot be read and a site that cannot be called the one in the earlier row is reported (in one row: the cell), as the
 * reference meets them: which error it is does not depend on group_rows.
 * out_ms8 (nullable): upload + index (host clock), index, parse, then id_markers: call, compact, -, -, download;
 * track_markers: matched sites, bit matrix, pairs, -, download (device events).
 * midas_sites_write_markers / _pairs: the two output tables formatted natively from these arrays and the tables' string columns
 * (site_id; sample_id of summary rows sample_row[s]); pairs in itertools.combinations order.                                  */
#define MIDAS_SITES_PAIR_TILE 64
int32_t midas_sites_id_markers(midas_snps_ctx* ctx, const char* freq, int64_t freq_bytes, const char* depth, int64_t depth_bytes,
                               int64_t n_parse, int64_t n_call, const uint8_t* minor_code, const uint8_t* major_code,
                               int32_t n_samples, const int32_t* sample_col, const double* fparams2, const int64_t* iparams8,
                               int32_t* out_rows7, int64_t* out_stats16, float* out_ms8);
int32_t midas_sites_track_markers(midas_snps_ctx* ctx, const char* freq, int64_t freq_bytes, const char* depth, int64_t depth_bytes,
                                  int64_t n_parse, int64_t n_call, const uint8_t* site_which, int32_t n_samples,
                                  const int32_t* sample_col, const double* fparams2, const int64_t* iparams8, int64_t* out_both,
                                  int64_t* out_stats16, float* out_ms8);
int32_t midas_sites_write_markers(const char* path, const midas_sites_tables* t, int64_t n_markers, const int32_t* rows7, char* err1024);
int32_t midas_sites_write_pairs(const char* path, const midas_sites_tables* t, int32_t n_samples, const int32_t* sample_row,
                                const int64_t* both, char* err1024);

/* ---- snp_trees.py: consensus distances between all pairs of samples, and a neighbour-joining tree over them --------------------
 * midas_sites_consensus_pairs walks the two matrices as midas_sites_scan does under MIDAS_SITES_SEQ (same text, masks, cell
 * parsers, row groups, site decisions, --max_sites rule and place of a bad row in out_stats16[4..6]); fparams5 as there (snp_maf
 * unused); iparams8 = site_depth, max_sites (-1: all), flags (MIDAS_SITES_MASK_ONLY alone is looked at), 0, group_rows,
 * chunk_bytes, pair_blocks (as midas_sites_track_markers), 0.  The retained sites of a row group become two bit planes [sample]
 * [64 sites a word]: `called` where call_consensus.py writes a letter (the sample is kept at the site and its depth is not 0),
 * `minor` where that letter is the minor allele (freq >= 0.5).  out_both / out_diff [n_samples][n_samples], filled for i <= j:
 * sites called in both samples, and those of them where one sample has the minor and the other the major allele.  Integer sums
 * held on the device across row groups: they depend on neither group_rows nor pair_blocks.  out_stats16: [0] sites read, [1]
 * sites retained, [2] / [3] cells converted by the host, [7] row groups, [8] (sample pairs with i <= j) x words of the planes,
 * [9] group_rows, [10] chunk_bytes, [11] / [12] the most word runs a pair launch had and the most staging steps a run had, [13]
 * the most samples whose pair matrices fit the free device memory (more is MIDAS_SNPS_ERR_OUT_OF_MEMORY).  out_ms8 (nullable):
 * upload + index (host clock), index, parse, site, planes, pairs, -, download (device events).
 * midas_nj_tree: neighbour joining over any symmetric matrix dist [n][n] of finite doubles (host memory), n >= 3, resident on the
 * device from the first step to the last.  Slots 0..n-1 are active and r = n; while r > 3, every operation one rounded fp64
 * operation as written:  R[a] = the sum of D[a][b] over the active b != a in ascending slot order, one add each from 0.0;
 * q = (((double)(r - 2) * D[a][b]) - R[a]) - R[b] for the active a < b; the pair with the least q is joined, compared by value,
 * ties to the smaller a, then the smaller b; la = 0.5 * D[a][b] + (R[a] - R[b]) / (2.0 * (double)(r - 2)), lb = D[a][b] - la
 * (negative lengths stay as they come); D[a][k] = D[k][a] = 0.5 * ((D[a][k] + D[b][k]) - D[a][b]) for the active k != a, b;
 * slot a holds the new node, slot b goes inactive, out_join[n - r] = (a, b), out_len[n - r] = (la, lb), r -= 1.  The last three
 * slots a < b < c: out_last = (a, b, c), out_last_len = 0.5 * ((D[a][b] + D[a][c]) - D[b][c]), 0.5 * ((D[a][b] + D[b][c]) -
 * D[a][c]), 0.5 * ((D[a][c] + D[b][c]) - D[a][b]).  The chosen pair never leaves the device between the launches of a step and
 * the host synchronises once, after the last step.  out_stats16: [0] the largest n the free device memory holds (more is
 * MIDAS_SNPS_ERR_OUT_OF_MEMORY), [1] steps, [2] kernel launches.  out_ms8 (nullable): upload, the steps, download.              */
int32_t midas_sites_consensus_pairs(midas_snps_ctx* ctx, const char* freq, int64_t freq_bytes, const char* depth, int64_t depth_bytes,
                                    int64_t n_sites_max, const uint8_t* site_mask, int32_t n_samples, const int32_t* sample_col,
                                    const double* mean_depth, const double* fparams5, const int64_t* iparams8, int64_t* out_both,
                                    int64_t* out_diff, int64_t* out_stats16, float* out_ms8);
int32_t midas_nj_tree(midas_snps_ctx* ctx, int32_t n, const double* dist, int32_t* out_join, double* out_len, int32_t* out_last,
                      double* out_last_len, int64_t* out_stats16, float* out_ms8);

/* ---- snp_pairs.py: pooled diversity, dxy and Fst of every pair of samples in one pass -------------------------------------------
 * Replaces scripts/snp_diversity.py:243-311 and midas/analyze/parse_snps.py:92-151, run once per pair with `--sample_type
 * pooled-samples --keep_samples a,b`.  midas_sites_pair_diversity walks the two matrices as midas_sites_scan does (same text,
 * masks, cell parsers, row groups, place of a bad row in out_stats16[4..6]); n_samples >= 2; fparams5 as there; iparams8 =
 * site_depth, max_sites (-1: all), flags (MIDAS_SITES_WEIGHT and MIDAS_SITES_ROUND are looked at; with MIDAS_SITES_WEIGHT
 * site_depth must be at least 1, so that no pool divides by 0), 0, group_rows, chunk_bytes, pair_form (0 or 1: one pair a
 * lane, tiles of 16 x 16 pairs; 2: a 4 x 4 patch a lane, tiles of 64 x 64; more is MIDAS_SNPS_ERR_INVALID_ARG), 0.  Every
 * (site, sample) cell is kept or not as flag_samples decides (site_depth, site_ratio, allele_support).  Then per pair i < j, over
 * the rows with site_mask set, in file order, a = f_i and b = f_j (rounded half to even under MIDAS_SITES_ROUND):
 *   count = kept cells of the two; pooled = 0.0 (count 0), else sum / count with sum = ((0.0 + a) + b) over the kept ones, or
 *   under MIDAS_SITES_WEIGHT ((0.0 + d_i a) + d_j b) / (d_i + d_j) over the kept ones; the site is retained unless site_prev != 0
 *   and count / 2 < max(1e-6, site_prev), or site_maf != 0 and pooled < site_maf, or the pair has retained max_sites sites;
 *   retained: sites += 1, pi += (2 pooled)(1 - pooled), snps += 1 where min(pooled, 1 - pooled) >= snp_maf (Python's min);
 *   retained and count 2: shared += 1, w1 += (2 a)(1 - a), w2 += (2 b)(1 - b), x += (a (1 - b)) + (b (1 - a)).
 * Every sum starts from +0.0 and takes one rounded fp64 operation per term, in site order: the results depend on neither
 * group_rows, chunk_bytes nor pair_form.  The seven outputs are [n_samples][n_samples], filled for i < j, 0 elsewhere.  Under
 * MIDAS_SITES_ROUND a frequency of a selected sample that is not finite, in any row, is MIDAS_SNPS_ERR_BAD_LAYOUT with
 * out_stats16[4] = 3; a malformed cell in any row is reported as midas_sites_scan reports it, whatever max_sites is.
 * out_stats16: [0] sites read, [1] rows with site_mask set, [2] / [3] cells converted by the host, [7] row groups, [8] pairs x
 * rows, [9] group_rows, [10] chunk_bytes, [11] pairs a lane a side (1 or 4), [12] tiles, [13] the most samples whose seven
 * matrices fit a quarter of the free device memory (more is MIDAS_SNPS_ERR_OUT_OF_MEMORY).  out_ms8 (nullable): upload + index
 * (host clock), index, parse, site, order, pairs, -, download (device events).                                                  */
int32_t midas_sites_pair_diversity(midas_snps_ctx* ctx, const char* freq, int64_t freq_bytes, const char* depth, int64_t depth_bytes,
                                   int64_t n_sites_max, const uint8_t* site_mask, int32_t n_samples, const int32_t* sample_col,
                                   const double* mean_depth, const double* fparams5, const int64_t* iparams8, int64_t* out_sites,
                                   int64_t* out_snps, int64_t* out_shared, double* out_pi, double* out_w1, double* out_w2,
                                   double* out_x, int64_t* out_stats16, float* out_ms8);

/* ---- snp_ld.py: linkage disequilibrium between pairs of sites, by distance ---------------------------------
 * midas_sites_ld walks the two matrices as midas_sites_consensus_pairs does (same text, masks, cell parsers, row groups, site
 * decisions under MIDAS_SITES_SEQ, --max_sites rule and place of a bad row in out_stats16[4..6]); fparams5 as there; iparams8 =
 * site_depth, max_sites (-1: all), flags (MIDAS_SITES_MASK_ONLY and MIDAS_SITES_LD_SAME_GENE are looked at), min_samples,
 * group_rows, chunk_bytes, anchor_chunk (0: what 256 MiB of per-anchor sums hold, at most 2^20), 0.  site_key [n_sites_max]: the
 * row's position, contig index * 2^40 + ref_pos, >= 0 and strictly ascending over the rows with site_mask set (else
 * MIDAS_SNPS_ERR_INVALID_ARG with the row in out_stats16[5]); site_gene [n_sites_max] (nullable without
 * MIDAS_SITES_LD_SAME_GENE): the row's gene index, -1 none.  1 <= max_dist < 2^39, bin_width >= 1, n_bins = ceil(max_dist /
 * bin_width) <= 4096.  For a retained site k and a sample s, `called` = the cell is kept and its depth is not 0, `minor` =
 * called and freq >= 0.5: the letters of call_consensus.py, held site-major [retained site][64 samples a word] on the device
 * for the whole call.
 * A pair is (a, b) of retained sites, a before b, with 1 <= key_b - key_a <= max_dist and, under MIDAS_SITES_LD_SAME_GENE, equal
 * gene indices >= 0; its bin is (key_b - key_a - 1) / bin_width.  With C the called and M the minor words, all int64:
 *   n = popc(C_a & C_b), na = popc(C_a & C_b & M_a), nb = popc(C_a & C_b & M_b), nab = popc(C_a & C_b & M_a & M_b)
 * window[bin] += 1 for every pair.  The pair is informative when n >= min_samples, 0 < na < n and 0 < nb < n; then pairs[bin] += 1
 * and, every line one rounded fp64 operation as written, without contraction:
 *   Dn = n*nab - na*nb, ha = na*(n - na), hb = nb*(n - nb)   (int64)
 *   num = (double)Dn * (double)Dn;  den = (double)ha * (double)hb;  r2 = num / den
 *   n2 = (double)(n*n);  n4 = n2 * n2;  d2 = num / n4;  het = den / n4
 * The sums have two serial levels: p_x[a][bin] (x = r2, d2, het) starts at +0.0 and takes one add per informative partner b of
 * that bin in ascending b; sum_x[bin] starts at +0.0 and takes one add of p_x[a][bin] per retained site a in ascending a.  So
 * the results depend on neither group_rows, chunk_bytes nor anchor_chunk.  out_window / out_pairs (int64) and out_sum_r2 /
 * out_sum_d2 / out_sum_het (double) are [n_bins].  out_stats16: [0] sites read, [1] sites retained, [2] / [3] cells converted by
 * the host, [7] row groups, [8] pairs visited, [9] group_rows, [10] chunk_bytes, [11] anchor chunks, [12] anchor_chunk, [13] the
 * most retained sites whose planes, keys and genes fit a quarter of the free device memory (more rows that CAN be retained --
 * rows with site_mask set, at most max_sites -- is MIDAS_SNPS_ERR_OUT_OF_MEMORY).  out_ms8 (nullable): upload + index (host
 * clock), index, parse, site, planes, LD kernel, fold, download (device events).                                                */
#define MIDAS_SITES_LD_SAME_GENE 128
int32_t midas_sites_ld(midas_snps_ctx* ctx, const char* freq, int64_t freq_bytes, const char* depth, int64_t depth_bytes,
                       int64_t n_sites_max, const uint8_t* site_mask, int32_t n_samples, const int32_t* sample_col,
                       const double* mean_depth, const double* fparams5, const int64_t* iparams8, const int64_t* site_key,
                       const int32_t* site_gene, int64_t max_dist, int64_t bin_width, int64_t* out_window, int64_t* out_pairs,
                       double* out_sum_r2, double* out_sum_d2, double* out_sum_het, int64_t* out_stats16, float* out_ms8);

/* ---- compare_genes.py: gene-content distances between all pairs of samples of one `merge_midas.py genes` directory ----------
 * midas_genes_matrix_*: one genes_<kind>.txt mapped and left as text.  counts: out4 = sample columns of the header, data rows
 *   (lines after the header; a last line without '\n' counts), bytes of those rows, bytes of the sample ids.  columns: out4 =
 *   the header's sample ids back to back (char), their offsets (int64, n + 1), the rows (char), the header's first field
 *   (char, *out_first_bytes long).  They belong to the handle.
 * midas_genes_compare: rows [0, n_rows_max) of `text` (the rows after the header, host memory); every row must have n_columns
 *   sample columns after its gene id, of which the first n_samples are used.  A cell is converted the way pandas' C reader
 *   converts it under read_table's defaults -- at most 17 digits accumulated in fp64, then ONE fp64 multiply or divide by a
 *   power of ten -- which is not float(); midas_genes_compare_parse_cell is that converter on the host (*out_plain_int: the
 *   cell has neither '.' nor an exponent).  A row of another width, or a cell among the used columns that is no finite decimal
 *   literal, is MIDAS_SNPS_ERR_BAD_LAYOUT with out_stats16[4] = 1 (width) or 2 (cell), [5] the 0-based data row, [6] the
 *   sample column (-1: width); the earliest in file order is reported, whatever the row groups are.
 *   MIDAS_GENES_PRESABS: a gene is present where its value > cutoff; out_count [n_samples][n_samples], filled for i <= j: genes
 *     present in both (the diagonal: in sample i).  Integers held on the device across row groups.
 *   MIDAS_GENES_COPYNUM: out_both / out_either [n_samples][n_samples], filled for i <= j: the sums of min(a, b) / max(a, b)
 *     over the rows IN ORDER, one fp64 add per row starting from 0, min = b < a ? b : a and max = b > a ? b : a (the
 *     diagonal of out_both: the sample's own sum); out_dist: the same sum of (a - b) * (a - b) (MIDAS_GENES_EUCLIDEAN, two
 *     roundings and the add) or |a - b| (MIDAS_GENES_MANHATTAN); unused under MIDAS_GENES_JACCARD.  The row axis is never split
 *     between workgroups or reduced in a tree and the sums carry across row groups in device memory: the bits do not depend
 *     on group_rows or chunk_bytes.
 *   out_col_float [n_samples]: 1 when some cell of the column has '.' or an exponent.  dump_cells (nullable, tests): the
 *   converted cells [n_samples][n_rows_max].  iparams4 = group_rows, chunk_bytes (0: from the free device memory), pair_blocks
 *   (presabs, as midas_sites_track_markers), 0.  out_stats16: [0] rows read, [7] row groups, [8] presabs: (pairs i <= j) x words,
 *   copynum: (pairs i <= j) x rows, [9] group_rows and [10] chunk_bytes in use, [11] pair tiles.  out_ms8 (nullable): upload +
 *   index (host clock), index, parse, bit matrix, pairs (popcount or ordered), -, -, download (device events).
 * midas_genes_compare_write_pairs: sample1, sample2, count1, count2, count_both, count_either, distance for every pair i < j in
 *   itertools.combinations order, numbers as str() writes them; n_rows = rows read (0: the sums are the integer 0).            */
#define MIDAS_GENES_PRESABS 0
#define MIDAS_GENES_COPYNUM 1
#define MIDAS_GENES_JACCARD 0
#define MIDAS_GENES_EUCLIDEAN 1
#define MIDAS_GENES_MANHATTAN 2
typedef struct midas_genes_matrix midas_genes_matrix;
int32_t midas_genes_matrix_open(const char* path, midas_genes_matrix** out, char* err1024);
int32_t midas_genes_matrix_counts(const midas_genes_matrix* m, int64_t* out4);
int32_t midas_genes_matrix_columns(const midas_genes_matrix* m, const void** out4, int64_t* out_first_bytes);
void midas_genes_matrix_close(midas_genes_matrix* m);
int32_t midas_genes_compare_parse_cell(const char* text, int64_t n, double* out, int32_t* out_plain_int);
int32_t midas_genes_compare(midas_snps_ctx* ctx, const char* text, int64_t text_bytes, int64_t n_rows_max, int32_t n_samples,
                            int32_t n_columns, int32_t dtype, int32_t distance, double cutoff, const int64_t* iparams4,
                            int64_t* out_count, double* out_both, double* out_either, double* out_dist, uint8_t* out_col_float,
                            double* dump_cells, int64_t* out_stats16, float* out_ms8);
int32_t midas_genes_compare_write_pairs(const char* path, const midas_genes_matrix* m, int32_t n_samples, int32_t dtype, int32_t distance,
                                        int64_t n_rows, const int64_t* count, const double* both, const double* either, const double* dist,
                                        char* err1024);

/* ---- gene_linkage.py: co-occurring pairs of genes and the groups they form -----------------------------
 * midas_genes_linkage reads the rows of genes_copynum.txt as midas_genes_compare does (same text, widths, cell converter, row
 *   groups, place of a bad row in out_stats16[4..6]).  Gene g is present in sample s when its value > cutoff; c_g counts the
 *   n_samples used samples in which it is.  g is kept when c_g >= min_present and n_samples - c_g >= min_absent; the kept genes get
 *   slots 0 .. K-1 in file order.  For slots a < b: both = popc(P_a & P_b) over the presence words (64 samples a word, pad bits
 *   0), either = c_a + c_b - both; the pair is linked when both >= need[either].  need [n_samples + 1] (int32) is the caller's:
 *   need[u] = the smallest n in [0, u] with (double)n / (double)u >= T, so the device holds no threshold and divides nothing.
 *   iparams8 = group_rows, chunk_bytes (0: from the free device memory), min_present (>= 1), min_absent (>= 0), pair_form (0: a
 *   partner's words in registers up to 16 words, 1: the form for any width), 0, 0, 0.
 *   out_count / out_row_of_slot / out_label [n_rows_max] (int32): the first K entries are c, the 0-based data row and the label of
 *   every slot; label[k] = the smallest slot of k's connected component in the graph of linked pairs (a singleton: k).
 *   out_a / out_b / out_both [max_pairs] (int32): the linked pairs, ascending a, then ascending b, with their `both`.  More than
 *   max_pairs (<= 2^31 - 1) linked pairs is MIDAS_SNPS_ERR_OUT_OF_MEMORY: out_stats16[11] holds the exact total and no output array
 *   is written.  Nothing depends on group_rows, chunk_bytes or pair_form.
 *   out_stats16: [0] rows read, [1] K, [4..6] a bad row, [7] row groups, [8] pairs visited K (K - 1) / 2, [9] group_rows and
 *   [10] chunk_bytes in use, [11] linked pairs, [12] label rounds that changed a label, [13] words a lane keeps in registers (0:
 *   the form for any width), [14] strips of 64 anchors.  out_ms8 (nullable): upload + index (host clock), index, parse, planes,
 *   count pass, write pass (with the scan of the row starts), labels, download (device events).
 * midas_genes_linkage_write_pairs: gene1, gene2, count1, count2, count_both, count_either, jaccard (repr of (double)both /
 *   (double)either) for the pairs in their order.  midas_genes_linkage_write_groups: group_id, group_size, gene_id, count for
 *   the slots of components of at least min_group slots; ids count from 1 in the order of the components' first genes, rows go
 *   by group, then by slot; *out_n_groups (nullable) = the groups written.                                                     */
int32_t midas_genes_linkage(midas_snps_ctx* ctx, const char* text, int64_t text_bytes, int64_t n_rows_max, int32_t n_samples,
                            int32_t n_columns, double cutoff, const int64_t* iparams8, const int32_t* need, int64_t max_pairs,
                            int32_t* out_count, int32_t* out_row_of_slot, int32_t* out_label, int32_t* out_a, int32_t* out_b,
                            int32_t* out_both, int64_t* out_stats16, float* out_ms8);
int32_t midas_genes_linkage_write_pairs(const char* path, const midas_genes_matrix* m, int64_t n_slots, const int32_t* count,
                                        const int32_t* row_of_slot, int64_t n_pairs, const int32_t* pair_a, const int32_t* pair_b,
                                        const int32_t* pair_both, char* err1024);
int32_t midas_genes_linkage_write_groups(const char* path, const midas_genes_matrix* m, int64_t n_slots, const int32_t* count,
                                         const int32_t* row_of_slot, const int32_t* label, int64_t min_group, int64_t* out_n_groups,
                                         char* err1024);

/* ---- gene_assoc.py: genes that differ between two groups of samples, with a permutation test ------------
 * midas_genes_assoc reads the rows of genes_copynum.txt as midas_genes_compare does (same text, widths, cell converter, row groups,
 *   place of a bad row in out_stats16[4..6]).  use_words / case_words [ceil(n_samples / 64)]: bit s set when column s takes part /
 *   is a case (a case bit outside use_words is ignored): N used samples, n1 cases.  More than 8 191 used samples is
 *   MIDAS_SNPS_ERR_UNSUPPORTED.  perm_planes [n_perms][ceil(n_samples / 64)]: bit s of plane b set when sample s is a case under
 *   relabelling b (the caller sets n1 bits among the used columns); n_perms <= 1 000 000; null only with n_perms 0.
 *   Presence is value > cutoff; c counts it over the used samples, a over the cases; a gene is kept when c >= min_present and
 *   N - c >= min_absent and gets the next slot in file order.  kind 0 (presabs): w = a, ties = 0, x(L) = N a(L) - n1 c.  kind 1
 *   (copynum): r_s = 2 #{t: v_t < v_s} + #{t: v_t == v_s} + 1 over the used samples, w = sum of r_s over the cases, ties = sum of
 *   (#{t: v_t == v_s}^2 - 1), x(L) = w(L) - n1 (N + 1).  exceed = #{b: |x(M_b)| >= |x(L0)|}.
 *   iparams8 = group_rows, chunk_bytes (0: from the free device memory), min_present, min_absent, kind, form (1: i8 MFMA; 0: one
 *   thread a (gene, relabelling), plain adds), 0, 0.
 *   out_row_of_slot / out_count / out_count_case (int32), out_w / out_ties (int64), out_exceed (uint32) [n_rows_max]: the first K
 *   entries are the slots'.  out_products (nullable, tests): int32 [min(n_rows_max * n_perms, 2^24)], a(M_b) or w(M_b) at
 *   slot * n_perms + b; MIDAS_SNPS_ERR_INVALID_ARG once K * n_perms exceeds 2^24.  Relabellings that take more than a quarter of
 *   the free device memory are MIDAS_SNPS_ERR_OUT_OF_MEMORY.  Nothing depends on group_rows, chunk_bytes or form.
 *   out_stats16: [0] rows read, [1] K, [4..6] a bad row, [7] row groups, [8] 1: the product kernel keeps a tile's digits in LDS,
 *   [9] group_rows and [10] chunk_bytes in use, [11] N, [12] n1, [13] form, [14] N rounded up to the K step.  out_ms8 (nullable):
 *   upload + index (host clock), index, parse, keep + ranks, product, expanding the relabellings, 0, download (device events).
 * midas_genes_assoc_write: gene_id, count_case, count_control, effect, p_value, q_value and, with n_perms > 0, exceed, p_perm,
 *   q_perm for the slots in their order (row_of_slot ascending); the doubles are the caller's, written as str() writes them. */
int32_t midas_genes_assoc(midas_snps_ctx* ctx, const char* text, int64_t text_bytes, int64_t n_rows_max, int32_t n_samples,
                          int32_t n_columns, const uint64_t* use_words, const uint64_t* case_words, const uint64_t* perm_planes,
                          int64_t n_perms, double cutoff, const int64_t* iparams8, int32_t* out_row_of_slot, int32_t* out_count,
                          int32_t* out_count_case, int64_t* out_w, int64_t* out_ties, uint32_t* out_exceed, int32_t* out_products,
                          int64_t* out_stats16, float* out_ms8);
int32_t midas_genes_assoc_write(const char* path, const midas_genes_matrix* m, int64_t n_slots, const int32_t* row_of_slot,
                                const int32_t* count, const int32_t* count_case, const double* effect, const double* p_value,
                                const double* q_value, int64_t n_perms, const uint32_t* exceed, const double* p_perm, const double* q_perm,
                                char* err1024);

/* ---- gene_curves.py: pangenome and core-genome accumulation curves over orders of the samples -----------
 * midas_genes_curves reads the rows of genes_copynum.txt as midas_genes_compare does (same text, widths, cell converter, row groups,
 *   place of a bad row in out_stats16[4..6]).  orders [n_orders][n_used] (int32): row 0 lists the n_used columns in use, every other
 *   row is a permutation of them; 1 <= n_orders <= 100 001, 1 <= n_used <= 8 191.  need [n_used + 1] (int32): need[k] = the fewest
 *   of the first k samples in which a core gene is present, 1 <= need[k] <= k (need[0] is not read).  Before any device work the
 *   entry point checks that every entry of orders is in [0, n_samples), that row 0 holds distinct entries, that every other row is
 *   a permutation of row 0's set and that need[] keeps its bounds: MIDAS_SNPS_ERR_INVALID_ARG with a message that names the row,
 *   and the outputs untouched.
 *   Presence is value > cutoff; c(g, r, k) = the number of the first k samples of order r in which gene g is present.
 *   out_pan / out_core / out_single [n_orders][n_used] (int64): at [r][k - 1] the genes with c >= 1, with c >= need[k], with
 *   c == 1, over every row read.  Orders and accumulators that take more than a quarter of the free device memory are
 *   MIDAS_SNPS_ERR_OUT_OF_MEMORY.  Nothing depends on group_rows, chunk_bytes or form.
 *   iparams8 = group_rows, chunk_bytes (0: from the free device memory), form (1: counts kept as bit planes over words of 64
 *   genes; 0: one thread a (order, gene), a plain count), 0, 0, 0, 0, 0.
 *   out_stats16: [0] rows read, [4..6] a bad row, [7] row groups, [8] words of 64 genes of the last group, [9] group_rows and
 *   [10] chunk_bytes in use, [11] n_used, [12] n_orders, [13] form, [14] counter planes a lane keeps (7, 10 or 13; form 0: 0).
 *   out_ms8 (nullable): upload + index (host clock), index, parse, planes, curves, 0, 0, download (device events).
 * midas_genes_curves_write: table 0: samples, pan, core, single, new (= pan[k] - pan[k - 1]) of order 0 for k = 1 .. n_used and,
 *   with n_perms > 0, pan_mean pan_min pan_max core_mean core_min core_max single_mean single_min single_max new_mean from means
 *   [4][n_used] (pan, core, single, new; written as str() writes them) and minmax [6][n_used] (int64: pan min, max, core min, max,
 *   single min, max).  table 1: order, samples, sample_id, pan, core, single for every (order, k); orders as above.            */
int32_t midas_genes_curves(midas_snps_ctx* ctx, const char* text, int64_t text_bytes, int64_t n_rows_max, int32_t n_samples,
                           int32_t n_columns, const int32_t* orders, int64_t n_orders, int32_t n_used, const int32_t* need, double cutoff,
                           const int64_t* iparams8, int64_t* out_pan, int64_t* out_core, int64_t* out_single, int64_t* out_stats16,
                           float* out_ms8);
int32_t midas_genes_curves_write(const char* path, const midas_genes_matrix* m, int32_t table, int64_t n_orders, int32_t n_used,
                                 const int64_t* pan, const int64_t* core, const int64_t* single, const int32_t* orders, int64_t n_perms,
                                 const double* means, const int64_t* minmax, char* err1024);

/* ---- run_species.py: the aligner's m8 lines classified (midas/run/species.py:51-119) -----------------------------------------
 * midas_species_classify: `text` (host memory) is the whole alignments.m8; it goes to the device chunk_bytes at a time and stays
 *   there.  A line's fields are its runs of non-blanks; query, target, pid (float), aln (int), score (float, field 12) are used and
 *   qlen = int() of the query's text after its last '_'.  pid and score are float() of their text, bit for bit: decoded on the
 *   device when the literal has at most 15 significant digits and a decimal exponent within +-22, by the host's parser
 *   otherwise.  The marker genes are gene_names[gene_name_off[g], gene_name_off[g + 1]) with their species and marker family
 *   (indices); a line passes unless pid < marker_cutoff[family] or (double)aln / qlen < aln_cov.  Per query (equal names, wherever
 *   the lines stand) the best hits are the passing lines whose score equals the query's maximum.  One best hit: out_uniq_reads /
 *   out_uniq_aln [n_species] take the read and its aln.  More: the query enters the result's CSR -- queries in the order of their
 *   first passing line, hits (species, aln) in line order -- for midas_species_assign.
 *   MIDAS_SNPS_ERR_BAD_LAYOUT with the 1-based number of the EARLIEST bad line in out_stats16[5] and the reason in [4]: 1 fewer
 *   than 12 fields, 2 a target that is no marker gene, 3 no usable qlen (zero included), 4 aln is no integer, 5 pid or score is no
 *   number, 6 the family's cutoff is nan (none given), 7 the score is nan.  aln and qlen beyond 32 bits are reasons 4 and 3.
 *   MIDAS_SNPS_ERR_UNSUPPORTED: a text beyond 4 GiB or 2^31 lines.
 *   iparams4 = chunk_bytes (0: 64 MiB; rounded up to 16), hash_bits (0 or 64: the whole hash of the query name; fewer, for tests,
 *   makes different names share a sort key -- the results do not change), dump (tests: the result keeps every line's decoded
 *   values for midas_species_result_lines), 0.  out_stats16: [0] lines, [1] passing lines, [2] unique reads, [3] ambiguous reads,
 *   [6] cells the host parsed, [7] chunks, [8] chunk_bytes in use, [9] hits of the ambiguous reads.  out_ms8 (nullable, host
 *   clock): upload, line index, fields, lookup, filter + sort + group, best hits, download.
 * midas_species_result_columns: indptr [ambiguous + 1], species and aln [hits].  _lines: per line pid, score, aln, qlen, species,
 *   marker (-1: no marker gene) and pass.
 * midas_species_assign (host only): the ambiguous reads given out one after another.  For a read with hits h_0..h_{k-1}:
 *   counts[i] = inout_reads[species of h_i]; all zero: index below k from getrandbits(k.bit_length()) of the first generator,
 *   redrawn until it is (random.sample(ids, 1)); else numpy's legacy choice with p = counts / sum: cdf = cumsum(p) / its last,
 *   u = ((a >> 5) * 2^26 + (b >> 6)) / 2^53 of two words of the second generator, the index is the number of cdf entries <= u.
 *   The drawn species gets the read and the aln of its FIRST hit in the list.  Both generators are MT19937: 624 words and the
 *   position (random.getstate()[1], np.random.get_state()[1:3]).  out_draws2 (nullable): words drawn from the first generator,
 *   doubles from the second.
 * midas_species_parse_number (tests): kind 0 float() -> double, 1 int() -> int64, as the classify step takes a field;
 *   *out_fast: the device's own decoder took it.                                                                              */
typedef struct midas_species_result midas_species_result;
int32_t midas_species_classify(midas_snps_ctx* ctx, const char* text, int64_t text_bytes, int32_t n_genes, const char* gene_names,
                               const int64_t* gene_name_off, const int32_t* gene_species, const int32_t* gene_marker, int32_t n_species,
                               int32_t n_markers, const double* marker_cutoff, double aln_cov, const int64_t* iparams4,
                               int64_t* out_uniq_reads, int64_t* out_uniq_aln, int64_t* out_stats16, float* out_ms8,
                               midas_species_result** out_result);
int32_t midas_species_result_columns(const midas_species_result* r, int64_t* indptr, int32_t* species, int32_t* aln);
int32_t midas_species_result_lines(const midas_species_result* r, double* pid, double* score, int32_t* aln, int32_t* qlen, int32_t* species,
                                   int32_t* marker, uint8_t* pass);
void midas_species_result_close(midas_species_result* r);
int32_t midas_species_assign(int64_t n_queries, const int64_t* indptr, const int32_t* hit_species, const int32_t* hit_aln, int32_t n_species,
                             const uint32_t* py_state624, int32_t py_pos, const uint32_t* np_state624, int32_t np_pos, int64_t* inout_reads,
                             int64_t* inout_aln, int64_t* out_draws2);
int32_t midas_species_parse_number(int32_t kind, const char* text, int64_t n, void* out, int32_t* out_fast);

/* ---- merge_species.py: the samples' species profiles merged (midas/merge/species.py:28-88) ---------------------------------------
 * midas_species_merge: profile_paths[s] is sample s's species/species_profile.txt; the library reads the files itself (host
 *   threads, groups of whole files of at most chunk_bytes of text, a larger file by itself), parses them on the device and keeps
 *   only the three [species][sample] matrices resident.  The species are species_ids[species_id_off[g], species_id_off[g + 1]),
 *   distinct, in the row order of species_info.txt.  A profile's header names its columns (species_id, count_reads, coverage,
 *   relative_abundance, anywhere; others are ignored); a line with another number of tab-separated fields than the header is
 *   skipped; cells are float() / int() of the field.  Per species over the samples in order: np.mean (pairwise add-reduce, one
 *   divide) and np.median of coverage and of relative abundance, each also as round(x, 2) of a numpy double (rint(x * 100) / 100),
 *   prevalence = samples with coverage >= sample_depth, and the species' place in a stable descending sort by prevalence.
 *   iparams4: chunk_bytes (0: 256 MiB), lds_bound (rows of at most this many samples are sorted in LDS, longer ones by the radix
 *   sort; 0 and anything above: 4096), host threads (0: the CPU budget), 0.
 *   out_stats16: [0] lines, [1] groups, [2] chunk_bytes, [3] cells the host's parser converted, [8] 1 = LDS rows, [9] lds_bound,
 *   [11] bytes of text; after MIDAS_SNPS_ERR_BAD_LAYOUT (the message names file, line and species or column; it is the earliest
 *   such line in the order of samples, then lines, a species without a line counting behind its profile's last line):
 *   [4] reason (1-4 the header lacks species_id / count_reads / coverage / relative_abundance, 5 species not in species_ids,
 *   6 species twice, 7-9 count_reads / coverage / relative_abundance does not convert, 10-11 coverage / relative_abundance not
 *   finite, 12 count_reads beyond int64, 13 a species without a line), [5] sample, [6] 1-based line, [7] species (reason 13).
 *   out_ms8: waiting for the readers, upload, index, fields, lookup + scatter, statistics, download.
 * _result_matrices: coverage, abundance (fp64) and reads (int64), each [n_species][n_samples].  _result_stats: stats8
 *   [8][n_species] = mean_coverage, median_coverage, mean_abundance, median_abundance, then the same four rounded; prevalence
 *   [n_species]; order [n_species] = the species of every row of species_prevalence.txt.
 * _result_write (host only): relative_abundance.txt, coverage.txt, count_reads.txt (header_line first, then a row a species:
 *   its id and str() of every cell) and species_prevalence.txt into outdir.                                                        */
typedef struct midas_species_merge_result midas_species_merge_result;
int32_t midas_species_merge(midas_snps_ctx* ctx, int32_t n_samples, const char* const* profile_paths, int32_t n_species, const char* species_ids,
                            const int64_t* species_id_off, double sample_depth, const int64_t* iparams4, int64_t* out_stats16, float* out_ms8,
                            midas_species_merge_result** out_result);
int32_t midas_species_merge_result_matrices(const midas_species_merge_result* r, double* coverage, double* abundance, int64_t* reads);
int32_t midas_species_merge_result_stats(const midas_species_merge_result* r, double* stats8, int64_t* prevalence, int32_t* order);
int32_t midas_species_merge_result_write(const midas_species_merge_result* r, const char* outdir, const char* header_line, int32_t threads,
                                         char* err1024);
void midas_species_merge_result_close(midas_species_merge_result* r);

/* ---- the exchange between ranks (comm.cpp): RCCL itself, no process group ------------------------------------------------
 * One process per GPU; the only thing ranks exchange on this path is the per-species summary rows -- the reference's pool
 * workers return (species_id, aln_stats) through a pipe, midas/run/snps.py:225-241, midas/utility.py:81-107 -- plus, on the
 * genes path, the (gene, term) pairs (midas/run/genes.py:165-199 computes them in one process).  librccl.so is loaded at run
 * time by the first of these calls (MIDAS_SNPS_ERR_UNSUPPORTED with the reason in err256 when it cannot be); a single-GPU run
 * never touches it.  Rank 0 makes the 128-byte id (ncclGetUniqueId) and hands it to the others however the caller likes
 * (midas_amd/dist.py: a file in <outdir>/snps/temp); every rank then joins with its context's device (ncclCommInitRank:
 * collective, returns when all have).  Buffers are the caller's host memory; the collective runs on the context's stream.
 *   all_gather     every rank's bytes_per_rank bytes, rank-major, to every rank (ncclAllGather over xGMI)
 *   all_to_all_v   send_bytes[r] bytes to rank r (taken from `send` back to back in rank order), recv_bytes[r] from rank r
 *                  (left in `recv` in rank order): grouped ncclSend / ncclRecv                                             */
typedef struct midas_comm midas_comm;
/* the PCI bus id of the context's device (two ranks on ONE device cannot form an RCCL communicator: the caller checks first) */
/* Whether this process can use RCCL at all (librccl loads and answers); *out_version: ncclGetVersion.  The ranks ask BEFORE they
 * call midas_comm_create together, and stay on their other transport if any of them cannot -- ncclCommInitRank waits for every
 * rank of the communicator, one that never arrives would hold the others there.                                                 */
int32_t midas_comm_probe(int32_t* out_version, char* err256);
int32_t midas_comm_device_key(midas_snps_ctx* ctx, char* out64);
int32_t midas_comm_unique_id(uint8_t* out_id128, char* err256);
int32_t midas_comm_create(midas_snps_ctx* ctx, const uint8_t* id128, int32_t rank, int32_t world, midas_comm** out, char* err256);
void midas_comm_destroy(midas_comm* comm);
int32_t midas_comm_all_gather(midas_comm* comm, const void* send, void* recv, int64_t bytes_per_rank, char* err256);
int32_t midas_comm_all_to_all_v(midas_comm* comm, const void* send, const int64_t* send_bytes, void* recv, const int64_t* recv_bytes,
                                char* err256);

/* The selected species' representative genomes read by all cores: initialize_contigs (midas/run/snps.py:55-67 -- Bio.SeqIO
 * over genome.fna[.gz], `str(rec.seq).upper()`).  Every file is read through zlib's gz layer (plain text passes through), cut
 * into records at the '>' that start a line (id = the header's first whitespace-separated word; what precedes the first header
 * is no record), whitespace removed, ASCII a-z upper-cased; the sequences of all files lie back to back in one pool, in file and
 * record order.  columns: out[0..5] = pool (uint8), rec_off (int64), rec_len (int64), rec_file (int32: index into paths), ids
 * (char, back to back), id_off (int64, n_records + 1); sizes[0..1] = bytes of the pool and of the ids.  They belong to the handle. */
typedef struct midas_fasta midas_fasta;
int32_t midas_fasta_load(int32_t n_files, const char* const* paths, int32_t threads, midas_fasta** out, char* err256);
int64_t midas_fasta_n_records(const midas_fasta* f);
int32_t midas_fasta_columns(const midas_fasta* f, const void** out, int64_t* sizes);
void midas_fasta_close(midas_fasta* f);

#ifdef __cplusplus
}
#endif
#endif /* MIDAS_SNPS_H */
