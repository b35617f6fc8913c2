// A resident batch of the C ABI (midas_snps_batch) and what the sources that implement it share: batch.hip (life cycle, run,
// results), batch_direct.hip, batch_packed.hip (the two fast paths' preparation and launches), batch_rows.hip (the table writer).
#pragma once
#include <algorithm>
#include <utility>
#include <vector>

#include "ctx_internal.h"
#include "kernels.h"
#include "layout.h"
#include "hostio.h"

// What the direct path's facts pass found (index_direct.hip, direct_facts_kernel), its slots added up.
struct DirectFactsSum {
  unsigned long long status = midas::kNoError, alg = 0, n_general = 0, n_long = 0, n_outliers = 0;
  uint32_t max_l = 0, max_span = 0, unsorted = 0, max_common = 0;
};

struct midas_snps_batch {
  midas_snps_ctx* ctx = nullptr;
  // Every device allocation of the batch (batch_alloc), freed by batch_destroy.  Pointers below that are NOT in it are borrowed:
  // a resident batch's columns and direct layout point into the BAM handle's device memory, its d_seq4 / d_qual / d_cigar into d_raw.
  std::vector<void*> owned;
  // device: the caller's BAM-native SoA, uploaded as it is (the device packer's input)
  int32_t *d_pos = nullptr, *d_nm = nullptr, *d_lseq = nullptr;
  uint8_t* d_mapq = nullptr;
  int64_t *d_seq_off = nullptr, *d_qual_off = nullptr, *d_cigar_off = nullptr;
  uint8_t *d_seq4 = nullptr, *d_qual = nullptr;
  uint32_t* d_cigar = nullptr;
  int64_t seq_bytes = 0, qual_bytes = 0, n_cigar = 0;
  // midas_snps_batch_create_resident: the reads are a run of a device-decoded BAM's records.  The columns above and the direct
  // layout below point INTO the BAM handle's device memory (the caller keeps the handle open); SEQ / QUAL / CIGAR as columns do
  // not exist until a path that reads them asks (ensure_raw_payload: cut out of the handle's inflated stream into d_raw, the
  // three pointers biased so that the BAM's absolute CSR offsets index them)
  bool resident = false;
  midas::ResidentReads rr;
  int64_t rr_first = 0;
  uint8_t* d_raw = nullptr;
  // the packer
  void* d_sort_tmp = nullptr;
  size_t sort_tmp_bytes = 0;
  int key_bits = 1;
  midas::PackParams pk;               // every pointer of a pack, filled once the buffers exist
  uint32_t* h_tile_reads = nullptr;   // pinned: reads every tile will see, fetched once per pack for the hot-spot plan
  std::vector<midas::Tile> h_tiles;   // the tile table as it was uploaded to d_tiles
  std::vector<int64_t> h_contig_site; // [n_contigs + 1] first site of every contig in d_counts / d_allele
  std::vector<int64_t> h_origin;      // [n_contigs] midas_snps_contigs.origin, empty when it was NULL
  std::vector<uint32_t> h_items;      // the work items last uploaded
  // device: the packed layout (layout.h)
  midas::ReadRec* d_rec = nullptr;
  uint8_t* d_blob = nullptr;
  uint8_t* d_ref = nullptr;
  midas::Tile* d_tiles = nullptr;
  int32_t *d_contig_read_begin = nullptr, *d_contig_tile_base = nullptr, *d_contig_len = nullptr;
  uint8_t* d_work = nullptr;  // [rbinv n_tiles][rend n_tiles][stats n_species*4 u64][err u64]
  midas::FilterTables* d_filt = nullptr;
  bool filt_fits16 = true;       // every entry of the tables fits 16 bits (the long-overhang instantiation of the direct kernel)
  uint32_t* d_orig = nullptr;   // device record -> input index (for error reports)
  uint32_t* d_key = nullptr;    // device record -> tile << 7 | reach << 2 | class (input of the index kernel)
  uint32_t* d_items = nullptr;  // [n_items][4] work items {tile, part, n_parts, 0} of the pileup kernel
  size_t items_cap = 0;         // words d_items can hold
  uint32_t* d_ticket = nullptr; // [n_tiles] arrival counters of split tiles
  bool has_high_qual = false;   // the payload holds a quality above kMaxPackedQual: a baseq above it cannot be served
  bool dense_clamped = false;   // the direct layout clamped an A/C/G/T quality above kDenseMaxQual (layout.h): a baseq above it goes the long way
  int64_t n_items = 0, n_whole_items = 0;
  std::vector<std::pair<size_t, size_t>> zero_ranges;   // (first site, sites) of split tiles: counts zeroed before a run
  midas::FilterTables h_filt;
  bool filt_valid = false;
  double filt_mapid = 0, filt_aln_cov = 0;
  int32_t max_l_seq = 0;
  uint32_t* d_counts = nullptr;
  uint8_t* d_allele = nullptr;
  // facts
  int64_t n_reads = 0, n_sites = 0, n_tiles = 0, blob_bytes = 0, alg_bytes = 0;
  int64_t n_records = 0;   // device records (match segments + reads that keep their CIGAR) >= n_reads
  int32_t n_contigs = 0, n_species = 0, lanes_per_read = 1, lane_bases = 31, tile_len = midas::kTileSites;
  // ---- direct path (index_direct.hip + pileup_direct.hip) ---------------------------------------------------------------
  int path = MIDAS_SNPS_PATH_DIRECT;   // the path batch_run takes
  int path_auto = MIDAS_SNPS_PATH_DIRECT;   // what the batch's own numbers recommend
  bool packed_built = false;    // rec / blob / orig / key exist (the packed path's layout is built on first use)
  uint32_t* d_trange = nullptr; // [2 parities][tbegin n_tiles][tend n_tiles]
  midas::DirectFacts* d_dfacts = nullptr;
  midas::DirectBlockCursor* d_block_contig = nullptr;   // per workgroup of the direct path's index kernels: the contig of its first read
  midas::DirectRec* d_drec = nullptr;  // [n_reads + 1] the direct layout: one 16-byte record per read ...
  uint8_t* d_dpay = nullptr;           // ... and its CIGAR / SEQ / QUAL bytes as one run (layout.h)
  int32_t layout_build_us = 0;         // device time of the layout's three launches (batch_get_info)
  // reads that span more than the overhang (a long deletion, an N skip): listed once (facts pass), so that the ranges pass keeps
  // to the common span and only the chunks they touch are dealt tile by tile
  midas::DirectOutlier* d_outliers = nullptr;
  uint32_t* d_n_outliers = nullptr;
  uint8_t* d_tile_flag = nullptr;
  uint8_t* d_chunk_ok = nullptr;       // per chunk of kDirectChunkTiles tiles (nullptr: every chunk carries its overhang)
  uint32_t outlier_cap = 0, n_outliers_listed = 0;
  int32_t direct_reach_ranges = 1;     // what the ranges pass reaches back over: the common span when the outliers are listed, else direct_reach
  int32_t direct_overhang = midas::kDirectOverhang;     // the batch's overhang: kDirectOverhangLong when its longest read asks for it (direct_prepare)
  bool direct_chunks = false;          // chunked tiles (position-sorted reads, outliers listed)
  unsigned long long* d_probe = nullptr;   // developer builds only (MIDAS_SNPS_DEBUG_BITS & 256)
  int64_t direct_general = 0;   // reads the pileup kernel walks op by op (facts pass)
  int32_t direct_reach = 1;     // longest reference span of a read: what a tile's range must reach back over
  int32_t direct_lane_bases = 30, direct_lanes_per_read = 1;      // (pileup_direct.hip direct_lane_bases: 30, 32 or 38)
  int64_t direct_stream_reads = 0;   // sum over tiles of the positions their streams hold (>= n_reads: straddlers twice)
  int64_t direct_max_tile_reads = 0;
  int64_t direct_run_count = 0;
  bool pad_advances = false;    // the context's pad rule when the batch was created (MIDAS_SNPS_PAD_PYSAM)
  int64_t n_long = 0;           // reads beyond the fast paths' limits: > 0 and the batch runs on the long path only (pileup_long.hip)
  DirectFactsSum direct_facts;  // the last facts pass, as it was summed (midas_snps_batch_fetch_index hands it out)
  bool direct_sorted = false;   // every contig's reads in position order (found by the first index pass): tile ranges need no atomics
  // timing
  std::vector<hipEvent_t> ev;  // 3 per slot: before the index kernel, before and after the pileup kernel
  std::vector<hipEvent_t> pev; // 3 per slot: before the pack, before and after its scatter kernel
  int32_t timing_slots = 0;
  bool timing_pileup_only = false;
  int64_t timed_runs = 0, timed_packs = 0;
  int64_t run_count = 0;
  bool ran = false;
};

// (internal to the library: none of it is an exported symbol)
namespace midas_batch MIDAS_INTERNAL {

// Device memory of the batch's own: recorded in b->owned, so batch_destroy frees it whatever happens in between.
template <class T>
inline hipError_t batch_alloc(midas_snps_batch* b, T** p, size_t bytes) {
  void* q = nullptr;
  const hipError_t e = hipMalloc(&q, bytes);
  if (e != hipSuccess) return e;
  b->owned.push_back(q);
  *p = static_cast<T*>(q);
  return hipSuccess;
}
// ... and given back early (the two buffers that regrow: d_items, d_sort_tmp)
template <class T>
inline void batch_release(midas_snps_batch* b, T** p) {
  const auto it = std::find(b->owned.begin(), b->owned.end(), static_cast<void*>(*p));
  if (it != b->owned.end()) { (void)hipFree(*it); b->owned.erase(it); }
  *p = nullptr;
}

// tile ranges of the packed path are double-buffered by run parity: [rbinv0][rend0][rbinv1][rend1]
// (each tile has three ranges, slots 3t..3t+2: see index_reads.hip)
inline uint32_t* work_rbinv(midas_snps_batch* b, int par) { return reinterpret_cast<uint32_t*>(b->d_work) + (size_t)par * 6 * b->n_tiles; }
inline uint32_t* work_rend(midas_snps_batch* b, int par) { return work_rbinv(b, par) + 3 * b->n_tiles; }
inline size_t work_stats_offset(int64_t n_tiles) { return ((size_t)n_tiles * 48 + 15) & ~(size_t)15; }
inline unsigned long long* work_stats(midas_snps_batch* b) { return reinterpret_cast<unsigned long long*>(b->d_work + work_stats_offset(b->n_tiles)); }
inline unsigned long long* work_err(midas_snps_batch* b) { return work_stats(b) + (size_t)b->n_species * midas::MIDAS_STATS; }
// ... and the direct path's: [2 parities][tbegin n_tiles][tend n_tiles]
inline uint32_t* trange_begin(midas_snps_batch* b, int par) { return b->d_trange + (size_t)par * 2 * (b->n_tiles > 0 ? b->n_tiles : 1); }
inline uint32_t* trange_end(midas_snps_batch* b, int par) { return trange_begin(b, par) + (b->n_tiles > 0 ? b->n_tiles : 1); }

// the ten raw columns, as every params struct that reads them names them (PackParams, DirectLayoutParams, LongParams)
template <class Params>
inline void fill_raw_columns(const midas_snps_batch* b, Params* p) {
  p->pos = b->d_pos; p->mapq = b->d_mapq; p->nm = b->d_nm; p->l_seq = b->d_lseq;
  p->seq_off = b->d_seq_off; p->qual_off = b->d_qual_off; p->cigar_off = b->d_cigar_off;
  p->seq4 = b->d_seq4; p->qual = b->d_qual; p->cigar = b->d_cigar;
}

int32_t pack_status_to_error(midas_snps_ctx* ctx, unsigned long long st);      // a facts pass's status word as the ABI's error
// batch_direct.hip
int32_t direct_prepare(midas_snps_batch* b);      // once per batch: buffers, facts, the layout, the choice of path
int32_t run_direct(midas_snps_batch* b, const midas_snps_thresholds* thr, hipEvent_t* ev);      // ev: the events of a timed run, or nullptr
// batch_packed.hip
int32_t ensure_raw_payload(midas_snps_batch* b);  // a resident batch's SEQ / QUAL / CIGAR as columns, cut on first use
int32_t ensure_packed(midas_snps_batch* b);       // the packed layout, built on first use
int32_t run_packed(midas_snps_batch* b, const midas_snps_thresholds* thr, hipEvent_t* ev);

}  // namespace midas_batch
