// The packed path of a batch: the device packer over the raw reads (pack_reads.hip), the hot-spot plan from the reads every
// tile will see (work_plan.h), and the index + pileup launches over the packed layout (index_reads.hip, pileup_tiles.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/midas_snps.h"
#include "batch.h"
#include "work_plan.h"

using namespace midas;
using namespace midas_ctx;
using namespace midas_batch;

namespace {

// The work plan of the reads every tile will see (work_plan.h), and its items on the device: uploaded only when a tile is split
// (with none the list is the identity and the kernel never reads it) and the plan differs from the one already there.
int32_t plan_work_items(midas_snps_batch* b) {
  midas_snps_ctx* ctx = b->ctx;
  WorkPlan plan = midas::plan_work_items(b->h_tile_reads, b->h_tiles.data(), (size_t)b->n_tiles, ctx->prop.multiProcessorCount, kWorkgroupsPerCU);
  b->n_whole_items = plan.n_whole;
  b->n_items = plan.n_items();
  b->zero_ranges.swap(plan.zero_ranges);
  if (!plan.any_split() || plan.items == b->h_items) return MIDAS_SNPS_OK;
  if (b->items_cap < plan.items.size()) {
    batch_release(b, &b->d_items);
    b->items_cap = 0;
    HIP_TRY(ctx, batch_alloc(b, &b->d_items, plan.items.size() * 4));
    b->items_cap = plan.items.size();
  }
  HIP_TRY(ctx, hipMemcpyAsync(b->d_items, plan.items.data(), plan.items.size() * 4, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  b->h_items.swap(plan.items);
  return MIDAS_SNPS_OK;
}

template <class T>
T* carve(uint8_t*& cur, size_t n) {
  T* r = reinterpret_cast<T*>(cur);
  cur += (n * sizeof(T) + 255) & ~(size_t)255;
  return r;
}
size_t carved(size_t n, size_t elem) { return (n * elem + 255) & ~(size_t)255; }


// The device packer over the resident raw reads, once the buffers exist: plan, keys, order, scatter on the context's stream.
// The per-tile read counts come back over a pinned buffer while the scatter kernel runs; the host derives the hot-spot
// plan from them (identical for identical input: nothing is uploaded then).
int32_t run_pack(midas_snps_batch* b, hipEvent_t* ev) {
  midas_snps_ctx* ctx = b->ctx;
  hipStream_t s = ctx->stream;
  if (ev) HIP_TRY(ctx, hipEventRecord(ev[0], s));
  HIP_TRY(ctx, launch_pack_plan(b->pk, b->d_sort_tmp, b->sort_tmp_bytes, s));
  HIP_TRY(ctx, launch_pack_keys(b->pk, s));
  HIP_TRY(ctx, launch_pack_order(b->pk, b->d_sort_tmp, b->sort_tmp_bytes, b->key_bits, s));
  if (b->n_tiles > 0)
    HIP_TRY(ctx, hipMemcpyAsync(b->h_tile_reads, b->pk.tile_reads, (size_t)b->n_tiles * 4, hipMemcpyDeviceToHost, s));
  if (ev) HIP_TRY(ctx, hipEventRecord(ev[1], s));
  HIP_TRY(ctx, launch_pack_scatter(b->pk, s));
  if (ev) HIP_TRY(ctx, hipEventRecord(ev[2], s));
  return MIDAS_SNPS_OK;
}

}  // namespace

// SEQ / QUAL / CIGAR of a resident batch as the three columns the packed and the long path read: cut out of the BAM handle's
// inflated stream on first use (bam_payload_kernel over the batch's records), into one buffer of the batch's own (d_raw); the
// pointers are biased by the first read's offsets, so the BAM's absolute CSR offsets index them.
int32_t midas_batch::ensure_raw_payload(midas_snps_batch* b) {
  if (!b->resident || b->d_raw || b->n_reads <= 0) return MIDAS_SNPS_OK;
  midas_snps_ctx* ctx = b->ctx;
  hipStream_t s = ctx->stream;
  long long lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
  const int64_t* offs[3] = {b->d_seq_off, b->d_qual_off, b->d_cigar_off};
  for (int k = 0; k < 3; ++k) {
    HIP_TRY(ctx, hipMemcpyAsync(&lo[k], offs[k], 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipMemcpyAsync(&hi[k], offs[k] + b->n_reads, 8, hipMemcpyDeviceToHost, s));
  }
  HIP_TRY(ctx, hipStreamSynchronize(s));
  auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
  const size_t sb = (size_t)(hi[0] - lo[0]), qb = (size_t)(hi[1] - lo[1]), cb = (size_t)(hi[2] - lo[2]) * 4;
  const size_t at_q = up(sb + 64), at_c = at_q + up(qb + 64), bytes = at_c + up(cb + 64);
  HIP_TRY(ctx, batch_alloc(b, &b->d_raw, bytes));
  uint8_t* base = b->d_raw;
  HIP_TRY(ctx, hipMemsetAsync(base + sb, 0, 64, s));
  HIP_TRY(ctx, hipMemsetAsync(base + at_q + qb, 0, 64, s));
  HIP_TRY(ctx, hipMemsetAsync(base + at_c + cb, 0, 64, s));
  b->d_seq4 = base - lo[0];
  b->d_qual = base + at_q - lo[1];
  b->d_cigar = reinterpret_cast<uint32_t*>(base + at_c) - lo[2];
  PayloadParams pp;
  pp.stream = b->rr.stream;
  pp.rec_off = reinterpret_cast<const unsigned long long*>(b->rr.rec_off) + b->rr_first;
  if (!b->rr.stream) {    // (a streamed decode: out of the direct layout, the side buffer's exact copies over the decoded bytes)
    pp.stream = b->rr.payload; pp.rec_off = nullptr; pp.drec = b->d_drec;
    pp.side = static_cast<const DenseSide*>(b->rr.side); pp.side_first = b->rr_first;
  }
  pp.n_records = b->n_reads;
  pp.seq_off = reinterpret_cast<const long long*>(b->d_seq_off); pp.qual_off = reinterpret_cast<const long long*>(b->d_qual_off);
  pp.cigar_off = reinterpret_cast<const long long*>(b->d_cigar_off);
  pp.seq4 = b->d_seq4; pp.qual = b->d_qual; pp.cigar = b->d_cigar;
  if (getenv("MIDAS_SNPS_TRACE"))
    fprintf(stderr, "[batch] raw columns cut out of %s: %lld reads, %zu + %zu + %zu bytes\n", pp.drec ? "the direct layout" : "the handle's inflated stream",
            (long long)b->n_reads, sb, qb, cb);
  HIP_TRY(ctx, launch_bam_payload(pp, ctx->prop.multiProcessorCount, s));
  return MIDAS_SNPS_OK;
}

// The packed path's device layout (layout.h), built on first use: plan, keys, order, scatter over the resident raw reads.
int32_t midas_batch::ensure_packed(midas_snps_batch* b) {
  if (b->packed_built) return MIDAS_SNPS_OK;
  midas_snps_ctx* ctx = b->ctx;
  if (b->n_long > 0) return fail(ctx, MIDAS_SNPS_ERR_UNSUPPORTED, "the batch holds reads beyond the packed layout's limits: it has the long path only");
  ST_TRY(ensure_raw_payload(b));
  hipStream_t s = ctx->stream;
  char ebuf[256] = {0};
  const int64_t n = b->n_reads, n_sites = b->n_sites;
  const size_t n1 = (size_t)(n > 0 ? n : 1);
  const size_t nt = (size_t)(b->n_tiles > 0 ? b->n_tiles : 1);
  // ---- packer, step 1: plan (validates every read on the device; the sizes come back) ----------------------------
  const size_t nbins = (size_t)b->n_tiles * kPackBinsPerTile + 1;
  {
    const size_t bytes = carved(n1, 1) + 2 * carved(n1 + 1, 4) + carved(kPackFactSlots, sizeof(PackFacts)) + carved(nbins, 4) + 2 * carved(nt, 4);
    uint8_t* cur = nullptr;      // (one slab per read: nseg, cnt, first, facts, bin_start, tile_extra, tile_reads)
    HIP_TRY(ctx, batch_alloc(b, &cur, bytes));
    PackParams& k = b->pk;
    memset(&k, 0, sizeof k);
    k.nseg = carve<uint8_t>(cur, n1);
    k.cnt = carve<uint32_t>(cur, n1 + 1);
    k.first = carve<uint32_t>(cur, n1 + 1);
    k.facts = carve<PackFacts>(cur, kPackFactSlots);
    k.bin_start = carve<uint32_t>(cur, nbins);
    k.tile_extra = carve<uint32_t>(cur, nt);
    k.tile_reads = carve<uint32_t>(cur, nt);
    fill_raw_columns(b, &k);
    k.seq_bytes = b->seq_bytes; k.qual_bytes = b->qual_bytes; k.n_cigar = b->n_cigar;
    k.n_reads = (int32_t)n;
    k.contig_read_begin = b->d_contig_read_begin; k.contig_tile_base = b->d_contig_tile_base; k.contig_len = b->d_contig_len;
    k.n_contigs = b->n_contigs; k.n_tiles = (int32_t)b->n_tiles; k.tile_len = b->tile_len; k.tile_shift = kTileShift;
    k.pad_advances = b->pad_advances ? 1 : 0;
  }
  b->key_bits = pack_key_bits((int32_t)b->n_tiles);
  // the first scan needs scratch before the record count is known: size it for the reads, regrow below for the records
  b->sort_tmp_bytes = pack_sort_temp_bytes((int64_t)n1 + 1, b->key_bits);
  HIP_TRY(ctx, batch_alloc(b, &b->d_sort_tmp, b->sort_tmp_bytes));
  HIP_TRY(ctx, launch_pack_plan(b->pk, b->d_sort_tmp, b->sort_tmp_bytes, s));
  PackFacts facts;
  std::vector<PackFacts> slots(kPackFactSlots);
  auto fetch_facts = [&]() -> hipError_t {   // the workgroups' partial sums, one slot per cache line
    hipError_t e = hipMemcpyAsync(slots.data(), b->pk.facts, sizeof(PackFacts) * kPackFactSlots, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    facts = slots[0];
    for (int k = 1; k < kPackFactSlots; ++k) {
      facts.alg_bytes += slots[k].alg_bytes;
      facts.blob_bytes += slots[k].blob_bytes;
      facts.n_records += slots[k].n_records;
      facts.max_l = std::max(facts.max_l, slots[k].max_l);
    }
    return e;
  };
  HIP_TRY(ctx, fetch_facts());
  if (facts.status != kNoError) ST_TRY(pack_status_to_error(ctx, facts.status));
  if (facts.n_records > 2000000000ull) {
    snprintf(ebuf, sizeof ebuf, "%llu device records exceed the supported range", facts.n_records);
    ST_TRY(fail(ctx, MIDAS_SNPS_ERR_UNSUPPORTED, ebuf));
  }
  const int64_t m = (int64_t)facts.n_records;
  b->n_records = m;
  b->max_l_seq = (int32_t)facts.max_l;
  b->alg_bytes = (int64_t)facts.alg_bytes + 17 * n_sites;
  b->lane_bases = lane_bases_for(b->max_l_seq);
  b->lanes_per_read = b->max_l_seq <= b->lane_bases ? 1 : (b->max_l_seq + b->lane_bases - 1) / b->lane_bases;

  // ---- packer, step 2: keys + sizes ------------------------------------------------------------------------------
  const size_t m1 = (size_t)(m > 0 ? m : 1);
  {
    const size_t bytes = 6 * carved(m1, 4) + 2 * carved(m1 + 1, 4) + carved(m1, 32);
    uint8_t* cur = nullptr;      // (one slab per record: sort keys / values (in + out), bytes8, dest, desc, bytes8_dev, off8)
    HIP_TRY(ctx, batch_alloc(b, &cur, bytes));
    PackParams& k = b->pk;
    k.sort_key = carve<uint32_t>(cur, m1);
    k.sort_val = carve<uint32_t>(cur, m1);
    k.key_sorted = carve<uint32_t>(cur, m1);
    k.val_sorted = carve<uint32_t>(cur, m1);
    k.bytes8 = carve<uint32_t>(cur, m1);
    k.dest = carve<uint32_t>(cur, m1);
    k.desc = carve<uint4>(cur, 2 * m1);
    k.bytes8_dev = carve<uint32_t>(cur, m1 + 1);
    k.off8 = carve<uint32_t>(cur, m1 + 1);
    k.n_records = (int32_t)m;
    k.lane_bases = b->lane_bases;
    k.lanes_per_read = b->lanes_per_read;
  }
  {
    const size_t need = pack_sort_temp_bytes((int64_t)std::max(m1, n1) + 1, b->key_bits);
    if (need > b->sort_tmp_bytes) {
      batch_release(b, &b->d_sort_tmp);
      HIP_TRY(ctx, batch_alloc(b, &b->d_sort_tmp, need));
      b->sort_tmp_bytes = need;
    }
  }
  HIP_TRY(ctx, launch_pack_keys(b->pk, s));
  HIP_TRY(ctx, fetch_facts());
  b->blob_bytes = (int64_t)facts.blob_bytes;
  if (facts.blob_bytes / 8 > 0xFFFFFFFFull) {
    snprintf(ebuf, sizeof ebuf, "packed payload %llu bytes exceeds the 32 GiB a batch can address", facts.blob_bytes);
    ST_TRY(fail(ctx, MIDAS_SNPS_ERR_UNSUPPORTED, ebuf));
  }

  // ---- packer, steps 3 + 4: device order, then records + payload ---------------------------------------------------
  const size_t blob_alloc = (size_t)b->blob_bytes + 64;  // slack: the last lane's 16-byte load may overhang
  HIP_TRY(ctx, batch_alloc(b, &b->d_rec, (size_t)(m + 1) * sizeof(ReadRec)));  // + sentinel
  HIP_TRY(ctx, batch_alloc(b, &b->d_blob, blob_alloc));
  HIP_TRY(ctx, batch_alloc(b, &b->d_orig, m1 * 4));
  HIP_TRY(ctx, batch_alloc(b, &b->d_key, m1 * 4));
  HIP_TRY(ctx, hipMemsetAsync(b->d_blob + b->blob_bytes, 0, 64, s));
  b->pk.rec = b->d_rec; b->pk.blob = b->d_blob; b->pk.orig = b->d_orig; b->pk.key_out = b->d_key;
  HIP_TRY(ctx, hipHostMalloc(reinterpret_cast<void**>(&b->h_tile_reads), nt * 4, kHostAllocFlags));
  HIP_TRY(ctx, launch_pack_order(b->pk, b->d_sort_tmp, b->sort_tmp_bytes, b->key_bits, s));
  if (b->n_tiles > 0)
    HIP_TRY(ctx, hipMemcpyAsync(b->h_tile_reads, b->pk.tile_reads, (size_t)b->n_tiles * 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(ctx, launch_pack_scatter(b->pk, s));
  HIP_TRY(ctx, fetch_facts());
  b->has_high_qual = slots[0].high_qual != 0;
  ST_TRY(plan_work_items(b));
  b->packed_built = true;
  return MIDAS_SNPS_OK;
}

extern "C" {

int32_t midas_snps_batch_pack(midas_snps_batch* b) {
  if (!b) return MIDAS_SNPS_ERR_INVALID_ARG;
  midas_snps_ctx* ctx = b->ctx;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (!b->packed_built) return ensure_packed(b);      // (building the layout IS a pack)
  hipEvent_t* ev = b->timing_slots > 0 ? &b->pev[(size_t)(b->timed_packs % b->timing_slots) * 3] : nullptr;
  ST_TRY(run_pack(b, ev));
  if (ev) b->timed_packs += 1;
  // the hot-spot plan needs the per-tile read counts on the host: one wait per pack (the scatter kernel is part of it)
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return plan_work_items(b);
}

int32_t midas_snps_batch_fetch_packed(midas_snps_batch* b, void* rec16, void* blob, uint32_t* orig_index, uint32_t* key,
                                      int64_t* out_n_records, int64_t* out_blob_bytes) {
  if (!b) return MIDAS_SNPS_ERR_INVALID_ARG;
  midas_snps_ctx* ctx = b->ctx;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  ST_TRY(ensure_packed(b));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (out_n_records) *out_n_records = b->n_records;
  if (out_blob_bytes) *out_blob_bytes = b->blob_bytes;
  if (rec16) HIP_TRY(ctx, hipMemcpy(rec16, b->d_rec, (size_t)(b->n_records + 1) * sizeof(ReadRec), hipMemcpyDeviceToHost));
  if (blob && b->blob_bytes > 0) HIP_TRY(ctx, hipMemcpy(blob, b->d_blob, (size_t)b->blob_bytes, hipMemcpyDeviceToHost));
  if (orig_index && b->n_records > 0) HIP_TRY(ctx, hipMemcpy(orig_index, b->d_orig, (size_t)b->n_records * 4, hipMemcpyDeviceToHost));
  if (key && b->n_records > 0) HIP_TRY(ctx, hipMemcpy(key, b->d_key, (size_t)b->n_records * 4, hipMemcpyDeviceToHost));
  return MIDAS_SNPS_OK;
}

}  // extern "C"

// A run on the packed path: the tile ranges from the records' keys, then the pileup kernel over whole tiles and parts.
int32_t midas_batch::run_packed(midas_snps_batch* b, const midas_snps_thresholds* thr, hipEvent_t* ev) {
  midas_snps_ctx* ctx = b->ctx;
  hipStream_t s = ctx->stream;
  ST_TRY(ensure_packed(b));
  const int par = (int)(b->run_count & 1);
  IndexParams ip;
  ip.rec = b->d_rec; ip.blob = b->d_blob; ip.key = b->d_key; ip.tiles = b->d_tiles;
  ip.rbinv = work_rbinv(b, par); ip.rend = work_rend(b, par);
  ip.rbinv_next = work_rbinv(b, par ^ 1); ip.rend_next = work_rend(b, par ^ 1);
  ip.n_tiles = (int32_t)b->n_tiles; ip.n_reads = (int32_t)b->n_records;
  ip.stats = work_stats(b); ip.err = work_err(b); ip.n_stat_words = b->n_species * MIDAS_STATS;
  ip.tile_len = b->tile_len; ip.lane_bases = b->lane_bases;
  HIP_TRY(ctx, launch_index_reads(ip, s));
  if (ev) HIP_TRY(ctx, hipEventRecord(ev[1], s));

  PileupParams pp;
  pp.rec = b->d_rec; pp.blob = b->d_blob; pp.ref = b->d_ref; pp.tiles = b->d_tiles;
  pp.rbinv = work_rbinv(b, par); pp.rend = work_rend(b, par);
  pp.out_counts = b->d_counts; pp.out_allele = b->d_allele;
  pp.stats = work_stats(b); pp.err = work_err(b);
  pp.items = b->d_items; pp.split_ticket = b->d_ticket;
  pp.n_items = (int32_t)b->n_items; pp.n_whole_items = (int32_t)b->n_whole_items;
  pp.n_tiles = (int32_t)b->n_tiles; pp.n_reads = (int32_t)b->n_records;
  pp.grid_blocks = ctx->prop.multiProcessorCount * kWorkgroupsPerCU;
#ifdef MIDAS_SNPS_GRID_BLOCKS   // developer variants only (tools/build_variant.sh)
  pp.grid_blocks = MIDAS_SNPS_GRID_BLOCKS;
#endif
  pp.lanes_per_read = b->lanes_per_read; pp.lane_bases = b->lane_bases; pp.reads_per_wave = 64 / b->lanes_per_read;
  pp.baseq = thr->baseq; pp.mapq = thr->mapq; pp.readq = thr->readq;
  pp.pad_advances = b->pad_advances ? 1 : 0;
  pp.filt = b->d_filt; pp.orig = b->d_orig; pp.table_len = b->max_l_seq + 1;
  for (const auto& zr : b->zero_ranges)   // split tiles accumulate with atomics: their counts start from zero
    HIP_TRY(ctx, hipMemsetAsync(b->d_counts + 4 * zr.first, 0, zr.second * 16, s));
  HIP_TRY(ctx, launch_pileup_tiles(pp, s, true, true));
  return MIDAS_SNPS_OK;
}
