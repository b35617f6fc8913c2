// Resident batches of the C ABI: create (the caller's arrays uploaded, or a device-decoded BAM's records used where they lie),
// destroy, the choice of path, runs, results and timing.  The paths' own work is batch_direct.hip, batch_packed.hip and, for the
// long path, run_long below.  See include/midas_snps.h for the contract and the reference lines each entry point replaces.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "../../include/midas_snps.h"
#include "batch.h"
#include "contigs.h"

using namespace midas;
using namespace midas_ctx;
using namespace midas_batch;

int32_t midas_batch::pack_status_to_error(midas_snps_ctx* ctx, unsigned long long st) {
  const long long rd = (long long)(st >> 8);
  char buf[256];
  ctx->err_read = rd;
  if ((st & 0xFF) == kPackUnsupported) {
    snprintf(buf, sizeof buf, "read %lld: l_seq > %d or n_cigar/NM > %d is not supported", rd, kMaxLSeq, kMaxField16);
    return fail(ctx, MIDAS_SNPS_ERR_UNSUPPORTED, buf);
  }
  snprintf(buf, sizeof buf, "read %lld: negative size or CSR offsets shorter than l_seq", rd);
  return fail(ctx, MIDAS_SNPS_ERR_BAD_LAYOUT, buf);
}

namespace {
#ifdef MIDAS_SNPS_TRACE   // developer variants only: where batch_create spends its time
struct CreateLap {
  std::chrono::steady_clock::time_point last = std::chrono::steady_clock::now();
  void operator()(const char* what) {
    const auto t = std::chrono::steady_clock::now();
    fprintf(stderr, "[batch_create] %-28s %8.2f ms\n", what, std::chrono::duration<double, std::milli>(t - last).count());
    last = t;
  }
};
#else
struct CreateLap { void operator()(const char*) {} };
#endif

// The tile table (tiles of kTileSites sites, the LDS budget: shorter tiles were measured and are slower) and the contig tables
// beside it, on the host and on the device.
int32_t upload_tile_table(midas_snps_batch* b, const midas_snps_contigs* contigs) {
  midas_snps_ctx* ctx = b->ctx;
  b->tile_len = kTileSites;
  const int64_t tile_len = b->tile_len;
  std::vector<Tile>& tiles = b->h_tiles;
  std::vector<int32_t> tile_base(contigs->n_contigs + 1, 0), clen(contigs->n_contigs), rbeg(contigs->n_contigs + 1, 0);
  int64_t site = 0;
  for (int32_t c = 0; c < contigs->n_contigs; ++c) {
    const int64_t len = contigs->length[c];
    tile_base[c] = (int32_t)tiles.size();
    clen[c] = (int32_t)len;
    rbeg[c] = (int32_t)contigs->read_begin[c];
    for (int64_t x = 0; x < len; x += tile_len) {
      Tile t;
      t.contig = c;
      t.start = (int32_t)x;
      t.len = (int32_t)((len - x) < tile_len ? (len - x) : tile_len);
      t.species = contigs->species[c];
      t.site_base = site + x;
      t.contig_len = (int32_t)len;
      t.halo = (contigs->origin && contigs->origin[c] > 0) ? 1 : 0;
      tiles.push_back(t);
    }
    site += len;
  }
  tile_base[contigs->n_contigs] = (int32_t)tiles.size();
  rbeg[contigs->n_contigs] = (int32_t)b->n_reads;
  b->h_contig_site.assign((size_t)contigs->n_contigs + 1, 0);
  for (int32_t c = 0; c < contigs->n_contigs; ++c) b->h_contig_site[(size_t)c + 1] = b->h_contig_site[(size_t)c] + contigs->length[c];
  if (contigs->origin) b->h_origin.assign(contigs->origin, contigs->origin + contigs->n_contigs);
  b->n_tiles = (int64_t)tiles.size();
  const size_t nt = (size_t)(b->n_tiles > 0 ? b->n_tiles : 1);
  HIP_TRY(ctx, batch_alloc(b, &b->d_tiles, nt * sizeof(Tile)));
  if (b->n_tiles > 0) HIP_TRY(ctx, hipMemcpy(b->d_tiles, tiles.data(), tiles.size() * sizeof(Tile), hipMemcpyHostToDevice));
  const size_t nc1 = (size_t)contigs->n_contigs + 1;
  HIP_TRY(ctx, batch_alloc(b, &b->d_contig_read_begin, nc1 * 4));
  HIP_TRY(ctx, batch_alloc(b, &b->d_contig_tile_base, nc1 * 4));
  HIP_TRY(ctx, batch_alloc(b, &b->d_contig_len, nc1 * 4));
  HIP_TRY(ctx, hipMemcpy(b->d_contig_read_begin, rbeg.data(), nc1 * 4, hipMemcpyHostToDevice));
  HIP_TRY(ctx, hipMemcpy(b->d_contig_tile_base, tile_base.data(), nc1 * 4, hipMemcpyHostToDevice));
  if (contigs->n_contigs > 0)
    HIP_TRY(ctx, hipMemcpy(b->d_contig_len, clen.data(), (size_t)contigs->n_contigs * 4, hipMemcpyHostToDevice));
  return MIDAS_SNPS_OK;
}

// The reads as they are: the packer runs on the device.
// (64 bytes of slack behind the byte arrays: the packer's 16-byte loads may overhang the last read)
int32_t upload_reads(midas_snps_batch* b, const midas_snps_reads* reads) {
  midas_snps_ctx* ctx = b->ctx;
  hipStream_t s = ctx->stream;
  const int64_t n = b->n_reads, seq_bytes = b->seq_bytes, qual_bytes = b->qual_bytes, n_cigar = b->n_cigar;
  const size_t n1 = (size_t)(n > 0 ? n : 1);
  HIP_TRY(ctx, batch_alloc(b, &b->d_pos, n1 * 4));
  HIP_TRY(ctx, batch_alloc(b, &b->d_mapq, n1));
  HIP_TRY(ctx, batch_alloc(b, &b->d_nm, n1 * 4));
  HIP_TRY(ctx, batch_alloc(b, &b->d_lseq, n1 * 4));
  HIP_TRY(ctx, batch_alloc(b, &b->d_seq_off, (n1 + 1) * 8));
  HIP_TRY(ctx, batch_alloc(b, &b->d_qual_off, (n1 + 1) * 8));
  HIP_TRY(ctx, batch_alloc(b, &b->d_cigar_off, (n1 + 1) * 8));
  HIP_TRY(ctx, batch_alloc(b, &b->d_seq4, (size_t)seq_bytes + 64));
  HIP_TRY(ctx, batch_alloc(b, &b->d_qual, (size_t)qual_bytes + 64));
  HIP_TRY(ctx, batch_alloc(b, &b->d_cigar, ((size_t)n_cigar + 16) * 4));
  if (n > 0) {
    // (a column that a device decode of this context copied down a moment ago and still holds -- the caller passes the decoder's
    // own read-only buffers, or a run of them -- is copied where it lies instead of going up the link again)
    auto column_up = [&](void* dst, const void* src, size_t bytes) -> hipError_t {
      const void* twin = ctx->arena->find_twin(src, bytes);
      return twin ? hipMemcpyAsync(dst, twin, bytes, hipMemcpyDeviceToDevice, s) : hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s);
    };
    HIP_TRY(ctx, column_up(b->d_pos, reads->pos, (size_t)n * 4));
    HIP_TRY(ctx, column_up(b->d_mapq, reads->mapq, (size_t)n));
    HIP_TRY(ctx, column_up(b->d_nm, reads->nm, (size_t)n * 4));
    HIP_TRY(ctx, column_up(b->d_lseq, reads->l_seq, (size_t)n * 4));
    HIP_TRY(ctx, column_up(b->d_seq_off, reads->seq_off, (size_t)(n + 1) * 8));
    HIP_TRY(ctx, column_up(b->d_qual_off, reads->qual_off, (size_t)(n + 1) * 8));
    HIP_TRY(ctx, column_up(b->d_cigar_off, reads->cigar_off, (size_t)(n + 1) * 8));
    // (seq4 / qual / cigar may be DEVICE pointers -- midas_bam_load_device leaves these columns there: the kind is inferred)
    if (seq_bytes > 0) HIP_TRY(ctx, hipMemcpyAsync(b->d_seq4, reads->seq4, (size_t)seq_bytes, hipMemcpyDefault, s));
    if (qual_bytes > 0) HIP_TRY(ctx, hipMemcpyAsync(b->d_qual, reads->qual, (size_t)qual_bytes, hipMemcpyDefault, s));
    if (n_cigar > 0) HIP_TRY(ctx, hipMemcpyAsync(b->d_cigar, reads->cigar, (size_t)n_cigar * 4, hipMemcpyDefault, s));
  }
  HIP_TRY(ctx, hipMemsetAsync(b->d_seq4 + seq_bytes, 0, 64, s));
  HIP_TRY(ctx, hipMemsetAsync(b->d_qual + qual_bytes, 0, 64, s));
  HIP_TRY(ctx, hipMemsetAsync(b->d_cigar + n_cigar, 0, 64, s));
  return MIDAS_SNPS_OK;
}

// Reference letters, workspace, outputs.
int32_t allocate_outputs(midas_snps_batch* b, const midas_snps_contigs* contigs) {
  midas_snps_ctx* ctx = b->ctx;
  hipStream_t s = ctx->stream;
  const size_t ns = (size_t)(b->n_sites > 0 ? b->n_sites : 1), nt = (size_t)(b->n_tiles > 0 ? b->n_tiles : 1);
  HIP_TRY(ctx, batch_alloc(b, &b->d_ref, ns));
  if (b->n_sites > 0) HIP_TRY(ctx, hipMemcpyAsync(b->d_ref, contigs->ref, (size_t)b->n_sites, hipMemcpyHostToDevice, s));
  const size_t work_bytes = work_stats_offset(b->n_tiles) + ((size_t)b->n_species * MIDAS_STATS + 1) * 8;
  HIP_TRY(ctx, batch_alloc(b, &b->d_work, work_bytes));
  // tile ranges start clean and every pileup workgroup re-zeroes its own entry; the counters and the
  // error word are reset by the index kernel at the start of each run: no per-run memsets
  HIP_TRY(ctx, hipMemsetAsync(b->d_work, 0, work_bytes, s));
  HIP_TRY(ctx, batch_alloc(b, &b->d_filt, sizeof(FilterTables)));
  HIP_TRY(ctx, batch_alloc(b, &b->d_counts, ns * 16));
  HIP_TRY(ctx, batch_alloc(b, &b->d_allele, ns));
  HIP_TRY(ctx, batch_alloc(b, &b->d_ticket, (nt + 2 * kSchedWords) * 4));     // + the two launches' dynamic-schedule words
  HIP_TRY(ctx, hipMemsetAsync(b->d_ticket, 0, (nt + 2 * kSchedWords) * 4, s));
  HIP_TRY(ctx, batch_alloc(b, &b->d_items, 4));
  b->items_cap = 1;
  return MIDAS_SNPS_OK;
}

// midas_snps_batch_create (reads: the caller's arrays, uploaded) and midas_snps_batch_create_resident (rbam: a device-decoded
// BAM whose records [first, first + contigs->read_begin[n_contigs]) are the batch's reads, used where they lie)
int32_t batch_create_impl(midas_snps_ctx* ctx, const midas_snps_contigs* contigs, const midas_snps_reads* reads, const midas_bam* rbam,
                          int64_t first, midas_snps_batch** out_batch) {
  if (!ctx || !contigs || (!reads && !rbam) || !out_batch) return MIDAS_SNPS_ERR_INVALID_ARG;
  *out_batch = nullptr;
  ctx->clear_error();
  ctx->err_read = -1;
  char ebuf[256] = {0};
  int64_t n_sites = 0;
  CreateLap lap;
  const midas::ResidentReads* rr = nullptr;
  int64_t r_total = 0, r_sb = 0, r_qb = 0, r_nc = 0;
  if (rbam) {
    rr = bam_resident(rbam, &r_total, &r_sb, &r_qb, &r_nc);
    if (!rr) return fail(ctx, MIDAS_SNPS_ERR_INVALID_ARG, "the BAM handle holds no device-resident records (midas_bam_load_resident)");
    if (contigs->n_contigs < 0 || (contigs->n_contigs > 0 && !contigs->read_begin)) return fail(ctx, MIDAS_SNPS_ERR_INVALID_ARG, "bad contig table header");
  }
  const int64_t n = rbam ? (contigs->n_contigs > 0 ? contigs->read_begin[contigs->n_contigs] : 0) : reads->n_reads;
  const int32_t st = validate_contigs(contigs, n, &n_sites, ebuf);
  if (st != MIDAS_SNPS_OK) return fail(ctx, st, ebuf);
  if (n < 0 || n > 2000000000LL) {
    snprintf(ebuf, sizeof ebuf, "n_reads %lld out of range", (long long)n);
    return fail(ctx, n < 0 ? MIDAS_SNPS_ERR_INVALID_ARG : MIDAS_SNPS_ERR_UNSUPPORTED, ebuf);
  }
  if (rbam && (first < 0 || first > r_total || n > r_total - first)) {
    snprintf(ebuf, sizeof ebuf, "records [%lld, %lld) lie outside the BAM handle's %lld", (long long)first, (long long)(first + n), (long long)r_total);
    return fail(ctx, MIDAS_SNPS_ERR_INVALID_ARG, ebuf);
  }
  if (!rbam && n > 0 && (!reads->pos || !reads->mapq || !reads->nm || !reads->l_seq || !reads->seq_off || !reads->qual_off ||
                         !reads->cigar_off || !reads->seq4 || !reads->qual || !reads->cigar))
    return fail(ctx, MIDAS_SNPS_ERR_INVALID_ARG, "NULL array in midas_snps_reads");
  // the CSR offsets' last entries are the array sizes (the device checks every read against them)
  const int64_t seq_bytes = rbam ? r_sb : (n > 0 ? reads->seq_off[n] : 0), qual_bytes = rbam ? r_qb : (n > 0 ? reads->qual_off[n] : 0),
                n_cigar = rbam ? r_nc : (n > 0 ? reads->cigar_off[n] : 0);
  if (!rbam && (seq_bytes < 0 || qual_bytes < 0 || n_cigar < 0 || (n > 0 && (reads->seq_off[0] < 0 || reads->qual_off[0] < 0 || reads->cigar_off[0] < 0))))
    return fail(ctx, MIDAS_SNPS_ERR_BAD_LAYOUT, "negative CSR offset in midas_snps_reads");

  HIP_TRY(ctx, hipSetDevice(ctx->device));
  // (the half-built batch is destroyed on every early return)
  struct Destroy { void operator()(midas_snps_batch* q) const { midas_snps_batch_destroy(q); } };
  std::unique_ptr<midas_snps_batch, Destroy> guard(new (std::nothrow) midas_snps_batch());
  midas_snps_batch* b = guard.get();
  if (!b) return fail(ctx, MIDAS_SNPS_ERR_OUT_OF_MEMORY, "host allocation failed");
  b->ctx = ctx;
  b->pad_advances = ctx->pad_rule == MIDAS_SNPS_PAD_PYSAM;
  b->n_reads = n;
  b->n_sites = n_sites;
  b->n_contigs = contigs->n_contigs;
  b->n_species = contigs->n_species;
  b->seq_bytes = seq_bytes;
  b->qual_bytes = qual_bytes;
  b->n_cigar = n_cigar;
  ST_TRY(upload_tile_table(b, contigs));
  lap("validate + tile table");
  if (rbam) {
    // the reads where the device decoder left them: the columns and the direct layout of the handle's records from `first` on
    b->resident = true;
    b->rr = *rr;
    b->rr_first = first;
    b->d_pos = rr->pos + first; b->d_mapq = rr->mapq + first; b->d_nm = rr->nm + first; b->d_lseq = rr->l_seq + first;
    b->d_seq_off = rr->seq_off + first; b->d_qual_off = rr->qual_off + first; b->d_cigar_off = rr->cigar_off + first;
    b->d_drec = static_cast<DirectRec*>(rr->rec) + first;
    b->d_dpay = rr->payload;
  } else {
    ST_TRY(upload_reads(b, reads));
  }
  lap("H2D raw reads");
  ST_TRY(allocate_outputs(b, contigs));
  lap("ref, workspace, outputs");
  // the direct path's index pass, once: validates every read on the device, sizes the general reads' descriptors, and tells how
  // well the reads are ordered (the path is chosen from that)
  ST_TRY(direct_prepare(b));
  lap("direct index (sizing run)");
  if (b->path == MIDAS_SNPS_PATH_PACKED) ST_TRY(ensure_packed(b));
  lap("packed layout");
  *out_batch = guard.release();
  return MIDAS_SNPS_OK;
}

// The long path: one thread per read over the raw columns (reads beyond the fast paths' limits; any batch may ask for it).
int32_t run_long(midas_snps_batch* b, const midas_snps_thresholds* thr, hipEvent_t* ev) {
  midas_snps_ctx* ctx = b->ctx;
  hipStream_t s = ctx->stream;
  ST_TRY(ensure_raw_payload(b));
  if (ev) HIP_TRY(ctx, hipEventRecord(ev[1], s));
  LongParams lp;
  fill_raw_columns(b, &lp);
  lp.n_reads = b->n_reads; lp.n_sites = b->n_sites;
  lp.contig_read_begin = b->d_contig_read_begin; lp.contig_tile_base = b->d_contig_tile_base;
  lp.n_contigs = b->n_contigs; lp.n_tiles = (int32_t)b->n_tiles;
  lp.tiles = b->d_tiles; lp.ref = b->d_ref;
  lp.out_counts = b->d_counts; lp.out_allele = b->d_allele;
  lp.stats = work_stats(b); lp.err = work_err(b);
  lp.n_stat_words = b->n_species * MIDAS_STATS;
  lp.baseq = thr->baseq; lp.mapq_min = thr->mapq; lp.readq = thr->readq; lp.pad_advances = b->pad_advances ? 1 : 0;
  lp.mapid = thr->mapid; lp.aln_cov = thr->aln_cov;
  HIP_TRY(ctx, launch_pileup_long(lp, s));
  return MIDAS_SNPS_OK;
}

// keep_read's fp64 ratio tests as exact integer thresholds on the device (rebuilt only when mapid / aln_cov change)
int32_t ensure_filter_tables(midas_snps_batch* b, const midas_snps_thresholds* thr) {
  midas_snps_ctx* ctx = b->ctx;
  if (b->filt_valid && memcmp(&b->filt_mapid, &thr->mapid, 8) == 0 && memcmp(&b->filt_aln_cov, &thr->aln_cov, 8) == 0) return MIDAS_SNPS_OK;
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // a previous run may still be reading the tables
  build_filter_tables(thr->mapid, thr->aln_cov, b->max_l_seq, &b->h_filt);
  HIP_TRY(ctx, hipMemcpy(b->d_filt, &b->h_filt, sizeof(FilterTables), hipMemcpyHostToDevice));
  b->filt_mapid = thr->mapid;
  b->filt_aln_cov = thr->aln_cov;
  b->filt_valid = true;
  // (the long-overhang instantiation of the direct kernel keeps these tables in 16 bits: an identity threshold so negative that a
  // table entry lies below -32768 -- mapid < -11 000 -- sends such a batch through the common instantiation, tile by tile)
  b->filt_fits16 = true;
  for (int32_t a = 0; a <= b->max_l_seq && a <= kMaxLSeq; ++a) b->filt_fits16 = b->filt_fits16 && b->h_filt.min_match[a] >= -32768 && b->h_filt.min_align[a] <= 32767;
  return MIDAS_SNPS_OK;
}
}  // namespace

extern "C" {

void midas_snps_batch_destroy(midas_snps_batch* b) {
  if (!b) return;
  if (b->ctx) (void)hipSetDevice(b->ctx->device);
  for (void* q : b->owned) (void)hipFree(q);
  if (b->h_tile_reads) (void)hipHostFree(b->h_tile_reads);
  for (auto& e : b->ev)
    if (e) (void)hipEventDestroy(e);
  for (auto& e : b->pev)
    if (e) (void)hipEventDestroy(e);
  delete b;
}

int32_t midas_snps_batch_create(midas_snps_ctx* ctx, const midas_snps_contigs* contigs,
                                const midas_snps_reads* reads, midas_snps_batch** out_batch) {
  if (!reads) return MIDAS_SNPS_ERR_INVALID_ARG;
  return batch_create_impl(ctx, contigs, reads, nullptr, 0, out_batch);
}

int32_t midas_snps_batch_create_resident(midas_snps_ctx* ctx, const midas_snps_contigs* contigs, const midas_bam* bam, int64_t first_read,
                                         midas_snps_batch** out_batch) {
  if (!bam) return MIDAS_SNPS_ERR_INVALID_ARG;
  return batch_create_impl(ctx, contigs, nullptr, bam, first_read, out_batch);
}

int32_t midas_snps_batch_select_path(midas_snps_batch* b, int32_t path) {
  if (!b || (path != MIDAS_SNPS_PATH_AUTO && path != MIDAS_SNPS_PATH_DIRECT && path != MIDAS_SNPS_PATH_PACKED && path != MIDAS_SNPS_PATH_LONG))
    return MIDAS_SNPS_ERR_INVALID_ARG;
  midas_snps_ctx* ctx = b->ctx;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (b->n_long > 0 && (path == MIDAS_SNPS_PATH_DIRECT || path == MIDAS_SNPS_PATH_PACKED)) {
    char buf[200];
    snprintf(buf, sizeof buf, "%lld read(s) with l_seq > %d or n_cigar / NM > %d: the batch has the long path only", (long long)b->n_long, kMaxLSeq, kMaxField16);
    return fail(ctx, MIDAS_SNPS_ERR_UNSUPPORTED, buf);
  }
  b->path = path == MIDAS_SNPS_PATH_AUTO ? b->path_auto : path;
  if (b->path == MIDAS_SNPS_PATH_PACKED) return ensure_packed(b);
  return MIDAS_SNPS_OK;
}

int32_t midas_snps_batch_enable_timing(midas_snps_batch* b, int32_t n_slots) {
  if (!b || n_slots < 0 || n_slots > 65536) return MIDAS_SNPS_ERR_INVALID_ARG;
  midas_snps_ctx* ctx = b->ctx;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  for (auto& e : b->ev)
    if (e) (void)hipEventDestroy(e);
  for (auto& e : b->pev)
    if (e) (void)hipEventDestroy(e);
  b->ev.assign((size_t)n_slots * 3, nullptr);
  b->pev.assign((size_t)n_slots * 3, nullptr);
  for (auto& e : b->ev) HIP_TRY(ctx, hipEventCreate(&e));
  for (auto& e : b->pev) HIP_TRY(ctx, hipEventCreate(&e));
  b->timing_slots = n_slots;
  b->timed_runs = 0;
  b->timed_packs = 0;
  return MIDAS_SNPS_OK;
}

int32_t midas_snps_batch_time_pileup_only(midas_snps_batch* b, int32_t on) {
  if (!b) return MIDAS_SNPS_ERR_INVALID_ARG;
  b->timing_pileup_only = on != 0;
  return MIDAS_SNPS_OK;
}

int32_t midas_snps_batch_run(midas_snps_batch* b, const midas_snps_thresholds* thr) {
  if (!b || !thr) return MIDAS_SNPS_ERR_INVALID_ARG;
  midas_snps_ctx* ctx = b->ctx;
  if (thr->reserved != 0) return fail(ctx, MIDAS_SNPS_ERR_INVALID_ARG, "thresholds.reserved must be 0");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  // The packed payload keeps a quality in six bits (exact for every threshold <= 62).  A baseq above that on reads that hold
  // qualities above it (BAM allows 93; Illumina tops out in the forties) is served by the direct kernel, which compares the
  // BAM's own bytes and is exact on any read order -- this one run only, the batch's path stays what it is.
  int run_path = b->path;
  if (run_path == MIDAS_SNPS_PATH_PACKED && thr->baseq > kMaxPackedQual) {
    ST_TRY(ensure_packed(b));
    if (b->has_high_qual) run_path = MIDAS_SNPS_PATH_DIRECT;
  }
  // The direct layout keeps an A/C/G/T quality in its base byte up to kDenseMaxQual (layout.h dense_byte): exact for every
  // baseq <= 50, and above that unless the batch holds a larger A/C/G/T quality (an absent QUAL's 0xFF included) -- that one
  // case is served by the long path over the raw columns, this run only.
  if (run_path == MIDAS_SNPS_PATH_DIRECT && thr->baseq > (int32_t)kDenseMaxQual && b->dense_clamped) run_path = MIDAS_SNPS_PATH_LONG;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  hipEvent_t* ev = b->timing_slots > 0 ? &b->ev[(size_t)(b->timed_runs % b->timing_slots) * 3] : nullptr;
  // an event record costs ~4 us of stream time (measured): a caller that only wants the pileup kernel's time leaves
  // the one in front of the index kernel out
  if (ev && !b->timing_pileup_only) HIP_TRY(ctx, hipEventRecord(ev[0], s));
  ST_TRY(ensure_filter_tables(b, thr));
  if (run_path == MIDAS_SNPS_PATH_LONG) ST_TRY(run_long(b, thr, ev));
  else if (run_path == MIDAS_SNPS_PATH_DIRECT) ST_TRY(run_direct(b, thr, ev));
  else ST_TRY(run_packed(b, thr, ev));
  if (ev) {
    HIP_TRY(ctx, hipEventRecord(ev[2], s));
    b->timed_runs += 1;
  }
  b->ran = true;
  b->run_count += 1;
  return MIDAS_SNPS_OK;
}

int32_t midas_snps_batch_sync(midas_snps_batch* b) {
  if (!b) return MIDAS_SNPS_ERR_INVALID_ARG;
  midas_snps_ctx* ctx = b->ctx;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (!b->ran) return MIDAS_SNPS_OK;
  unsigned long long e = kNoError;
  HIP_TRY(ctx, hipMemcpy(&e, work_err(b), 8, hipMemcpyDeviceToHost));
  if (e != kNoError) {
    const int32_t kind = (int32_t)(e & 0xFF);
    ctx->err_read = (int64_t)(e >> 8);
    char buf[256];
    snprintf(buf, sizeof buf, "read %lld: %s", (long long)ctx->err_read, read_err_name(kind));
    return fail(ctx, kind, buf);
  }
  return MIDAS_SNPS_OK;
}

int32_t midas_snps_batch_fetch(midas_snps_batch* b, uint32_t* out_counts, uint8_t* out_allele, int64_t* out_stats) {
  int32_t st = midas_snps_batch_sync(b);
  if (st != MIDAS_SNPS_OK) return st;
  midas_snps_ctx* ctx = b->ctx;
  if (!b->ran) return fail(ctx, MIDAS_SNPS_ERR_INVALID_ARG, "batch_fetch before batch_run");
  if (out_counts && b->n_sites > 0) {
    st = copy_to_host(ctx, out_counts, b->d_counts, (size_t)b->n_sites * 16);
    if (st != MIDAS_SNPS_OK) return st;
  }
  if (out_allele && b->n_sites > 0) {
    st = copy_to_host(ctx, out_allele, b->d_allele, (size_t)b->n_sites);
    if (st != MIDAS_SNPS_OK) return st;
  }
  if (out_stats && b->n_species > 0)
    HIP_TRY(ctx, hipMemcpy(out_stats, work_stats(b), (size_t)b->n_species * MIDAS_STATS * 8, hipMemcpyDeviceToHost));
  return MIDAS_SNPS_OK;
}

#if MIDAS_SNPS_DEBUG_BITS & 256
// developer builds only: the direct pileup kernel's per-wave cycle counts of the last run (8 words per wave)
int32_t midas_snps_debug_probe(midas_snps_batch* b, unsigned long long* out, int64_t n_words) {
  if (!b || !out || !b->d_probe) return MIDAS_SNPS_ERR_INVALID_ARG;
  const int64_t have = (int64_t)b->ctx->prop.multiProcessorCount * kWorkgroupsPerCU * (kPileupBlock / 64) * 8;
  HIP_TRY(b->ctx, hipDeviceSynchronize());
  HIP_TRY(b->ctx, hipMemcpy(out, b->d_probe, (size_t)std::min(have, n_words) * 8, hipMemcpyDeviceToHost));
  return MIDAS_SNPS_OK;
}
#endif

int32_t midas_snps_batch_get_info(const midas_snps_batch* b, midas_snps_batch_info* out) {
  if (!b || !out) return MIDAS_SNPS_ERR_INVALID_ARG;
  out->n_reads = b->n_reads;
  out->n_sites = b->n_sites;
  out->n_tiles = b->n_tiles;
  out->packed_bytes = b->packed_built ? b->blob_bytes + b->n_records * (int64_t)sizeof(ReadRec) : 0;
  out->algorithmic_bytes = b->alg_bytes;
  out->tile_sites = b->tile_len;
  out->lanes_per_read = b->path == MIDAS_SNPS_PATH_DIRECT ? b->direct_lanes_per_read : b->lanes_per_read;
  out->n_work_items = b->path == MIDAS_SNPS_PATH_DIRECT ? b->n_tiles : b->n_items;
  out->path = b->path;
  out->path_auto = b->path_auto;
  out->lane_bases = b->path == MIDAS_SNPS_PATH_DIRECT ? b->direct_lane_bases : b->lane_bases;
  out->layout_build_us = b->layout_build_us;
  out->direct_general_reads = b->direct_general;
  out->direct_reach = b->direct_reach;
  out->direct_stream_reads = b->direct_stream_reads;
  out->direct_max_tile_reads = b->direct_max_tile_reads;
  out->direct_chunk_tiles = b->direct_chunks ? kDirectChunkTiles : 1;
  out->direct_overhang = b->direct_chunks ? b->direct_overhang : kDirectOverhang;
  return MIDAS_SNPS_OK;
}

int32_t midas_snps_batch_timing(midas_snps_batch* b, int32_t slot, float out_ms[3]) {
  if (!b || !out_ms) return MIDAS_SNPS_ERR_INVALID_ARG;
  midas_snps_ctx* ctx = b->ctx;
  if (slot < 0 || slot >= b->timing_slots || slot >= b->timed_runs)
    return fail(ctx, MIDAS_SNPS_ERR_INVALID_ARG, "no timed run recorded in that slot");
  hipEvent_t* ev = &b->ev[(size_t)slot * 3];
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipEventSynchronize(ev[2]));
  HIP_TRY(ctx, hipEventElapsedTime(&out_ms[1], ev[1], ev[2]));
  if (b->timing_pileup_only) {
    out_ms[0] = 0.f;
    out_ms[2] = out_ms[1];
  } else {
    HIP_TRY(ctx, hipEventElapsedTime(&out_ms[0], ev[0], ev[1]));
    HIP_TRY(ctx, hipEventElapsedTime(&out_ms[2], ev[0], ev[2]));
  }
  return MIDAS_SNPS_OK;
}

int32_t midas_snps_batch_pack_timing(midas_snps_batch* b, int32_t slot, float out_ms[2]) {
  if (!b || !out_ms) return MIDAS_SNPS_ERR_INVALID_ARG;
  midas_snps_ctx* ctx = b->ctx;
  if (slot < 0 || slot >= b->timing_slots || slot >= b->timed_packs)
    return fail(ctx, MIDAS_SNPS_ERR_INVALID_ARG, "no timed pack recorded in that slot");
  hipEvent_t* ev = &b->pev[(size_t)slot * 3];
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipEventSynchronize(ev[2]));
  HIP_TRY(ctx, hipEventElapsedTime(&out_ms[0], ev[0], ev[2]));
  HIP_TRY(ctx, hipEventElapsedTime(&out_ms[1], ev[1], ev[2]));
  return MIDAS_SNPS_OK;
}

int32_t midas_snps_batch_stats_to_device(midas_snps_batch* b, void* dst) {
  if (!b || !dst) return MIDAS_SNPS_ERR_INVALID_ARG;
  midas_snps_ctx* ctx = b->ctx;
  if (!b->ran) return fail(ctx, MIDAS_SNPS_ERR_INVALID_ARG, "stats_to_device before batch_run");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (b->n_species > 0)
    HIP_TRY(ctx, hipMemcpyAsync(dst, work_stats(b), (size_t)b->n_species * MIDAS_STATS * 8, hipMemcpyDeviceToDevice,
                                ctx->stream));
  return MIDAS_SNPS_OK;
}

int32_t midas_snps_pileup(midas_snps_ctx* ctx, const midas_snps_thresholds* thr, const midas_snps_contigs* contigs,
                          const midas_snps_reads* reads, uint32_t* out_counts, uint8_t* out_allele,
                          int64_t* out_stats) {
  if (!ctx || !thr) return MIDAS_SNPS_ERR_INVALID_ARG;
  midas_snps_batch* b = nullptr;
  int32_t st = midas_snps_batch_create(ctx, contigs, reads, &b);
  if (st != MIDAS_SNPS_OK) return st;
  st = midas_snps_batch_run(b, thr);
  if (st == MIDAS_SNPS_OK) st = midas_snps_batch_fetch(b, out_counts, out_allele, out_stats);
  midas_snps_batch_destroy(b);
  return st;
}

}  // extern "C"
