// The direct path of a batch (index_direct.hip + pileup_direct.hip): its preparation, once per batch -- every read validated on
// the device, the batch's totals, the direct layout, one ranges pass and the choice of path from its numbers -- and its runs.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/midas_snps.h"
#include "batch.h"

using namespace midas;
using namespace midas_ctx;
using namespace midas_batch;

namespace {

void fill_direct_index(midas_snps_batch* b, DirectIndexParams* ip) {
  const int par = (int)(b->direct_run_count & 1);
  ip->pos = b->d_pos; ip->nm = b->d_nm; ip->l_seq = b->d_lseq;
  ip->seq_off = b->d_seq_off; ip->qual_off = b->d_qual_off; ip->cigar_off = b->d_cigar_off;
  ip->cigar = b->d_cigar;
  ip->rec = b->resident ? b->d_drec : nullptr;          // (a resident batch has no CIGAR column: the facts pass reads the ops in the payload)
  ip->payload = b->resident ? b->d_dpay : nullptr;
  ip->seq_bytes = b->seq_bytes; ip->qual_bytes = b->qual_bytes; ip->n_cigar = b->n_cigar;
  ip->n_reads = (int32_t)b->n_reads;
  ip->contig_read_begin = b->d_contig_read_begin; ip->contig_tile_base = b->d_contig_tile_base; ip->contig_len = b->d_contig_len;
  ip->n_contigs = b->n_contigs; ip->n_tiles = (int32_t)b->n_tiles; ip->tile_shift = kTileShift;
  ip->tbegin = trange_begin(b, par); ip->tend = trange_end(b, par);
  ip->tbegin_next = trange_begin(b, par ^ 1); ip->tend_next = trange_end(b, par ^ 1);
  ip->sorted = b->direct_sorted ? 1 : 0;
  ip->reach = b->direct_reach_ranges;
  ip->overhang = b->direct_overhang;
  ip->outliers = b->d_outliers; ip->n_outliers_listed = b->d_n_outliers; ip->outlier_cap = b->outlier_cap;
  ip->tile_flag = b->d_tile_flag;
  ip->facts = b->d_dfacts;
  ip->block_contig = b->d_block_contig;
  ip->stats = b->d_work ? work_stats(b) : nullptr; ip->err = b->d_work ? work_err(b) : nullptr;
  ip->n_stat_words = b->d_work ? b->n_species * MIDAS_STATS : 0;
}

// The facts pass starts from clean cursors, fact slots (status words at "no error"), outlier count and tile flags.
int32_t reset_facts(midas_snps_batch* b) {
  midas_snps_ctx* ctx = b->ctx;
  hipStream_t s = ctx->stream;
  const size_t nt = (size_t)(b->n_tiles > 0 ? b->n_tiles : 1);
  HIP_TRY(ctx, hipMemsetAsync(b->d_block_contig, 0, (size_t)direct_index_blocks(b->n_reads) * sizeof(DirectBlockCursor), s));
  HIP_TRY(ctx, hipMemsetAsync(b->d_dfacts, 0, sizeof(DirectFacts) * kDirectFactSlots, s));
  for (int k = 0; k < kDirectFactSlots; ++k) HIP_TRY(ctx, hipMemsetAsync(&b->d_dfacts[k].status, 0xFF, 8, s));
  HIP_TRY(ctx, hipMemsetAsync(b->d_n_outliers, 0, 4, s));
  HIP_TRY(ctx, hipMemsetAsync(b->d_tile_flag, 0, nt, s));
  return MIDAS_SNPS_OK;
}

// step 1: the direct path's buffers; tile bounds start clean (every pass resets the other parity's)
int32_t allocate_and_reset(midas_snps_batch* b) {
  midas_snps_ctx* ctx = b->ctx;
  hipStream_t s = ctx->stream;
  const size_t nt = (size_t)(b->n_tiles > 0 ? b->n_tiles : 1);
  b->outlier_cap = (uint32_t)std::max<int64_t>(4096, b->n_reads / 64);
  HIP_TRY(ctx, batch_alloc(b, &b->d_trange, nt * 4 * 4));
  HIP_TRY(ctx, batch_alloc(b, &b->d_dfacts, sizeof(DirectFacts) * kDirectFactSlots));
  HIP_TRY(ctx, batch_alloc(b, &b->d_block_contig, (size_t)direct_index_blocks(b->n_reads) * sizeof(DirectBlockCursor)));
  HIP_TRY(ctx, batch_alloc(b, &b->d_outliers, (size_t)b->outlier_cap * sizeof(DirectOutlier)));
  HIP_TRY(ctx, batch_alloc(b, &b->d_n_outliers, 4));
  HIP_TRY(ctx, batch_alloc(b, &b->d_tile_flag, nt));
  HIP_TRY(ctx, hipMemsetAsync(b->d_trange, 0, nt * 16, s));
  HIP_TRY(ctx, hipMemsetAsync(trange_begin(b, 0), 0xFF, nt * 4, s));
  HIP_TRY(ctx, hipMemsetAsync(trange_begin(b, 1), 0xFF, nt * 4, s));
  return reset_facts(b);
}

using FactsSum = DirectFactsSum;      // (batch.h: the batch keeps the last one)
int32_t facts_pass(midas_snps_batch* b, FactsSum* sum) {
  midas_snps_ctx* ctx = b->ctx;
  hipStream_t s = ctx->stream;
  DirectIndexParams ip;
  fill_direct_index(b, &ip);
  if (b->n_reads > 0) HIP_TRY(ctx, launch_direct_facts(ip, s));
  std::vector<DirectFacts> facts(kDirectFactSlots);
  HIP_TRY(ctx, hipMemcpyAsync(facts.data(), b->d_dfacts, sizeof(DirectFacts) * kDirectFactSlots, hipMemcpyDeviceToHost, s));
  HIP_TRY(ctx, hipStreamSynchronize(s));
  *sum = FactsSum{};
  for (const DirectFacts& f : facts) {
    sum->n_outliers += f.n_outliers;
    sum->max_common = std::max(sum->max_common, f.max_span_common);
    sum->status = std::min(sum->status, f.status);
    sum->alg += f.alg_bytes;
    sum->n_general += f.n_general;
    sum->n_long += f.n_long;
    sum->max_l = std::max(sum->max_l, f.max_l);
    sum->max_span = std::max(sum->max_span, f.max_span);
    sum->unsorted |= f.unsorted;
  }
  return sum->status == kNoError ? MIDAS_SNPS_OK : pack_status_to_error(ctx, sum->status);
}

// step 2: the facts pass (twice when the batch's longest read asks for the long overhang) and what the batch keeps of it
int32_t facts_and_summary(midas_snps_batch* b) {
  midas_snps_ctx* ctx = b->ctx;
  const size_t nt = (size_t)(b->n_tiles > 0 ? b->n_tiles : 1);
  FactsSum f;
  b->direct_overhang = kDirectOverhang;
  ST_TRY(facts_pass(b, &f));
  // Reads longer than the common overhang (250 bp reads), position-sorted: the batch takes the kernel's instantiation with the
  // long overhang -- and which reads are OUTLIERS is a question of that overhang: the facts pass again (once per batch, a few ms).
  static const int overhang_max = [] { const char* e = getenv("MIDAS_SNPS_OVERHANG_MAX"); return e ? atoi(e) : kDirectOverhangLong; }();
  if (kDirectChunkTiles > 1 && f.unsorted == 0 && f.n_long == 0 && f.max_l > (uint32_t)kDirectOverhang && f.max_l <= (uint32_t)kDirectOverhangLong &&
      overhang_max >= kDirectOverhangLong) {
    b->direct_overhang = kDirectOverhangLong;
    ST_TRY(reset_facts(b));
    ST_TRY(facts_pass(b, &f));
  }
  b->direct_facts = f;
  b->max_l_seq = (int32_t)f.max_l;
  b->direct_sorted = f.unsorted == 0;
  b->direct_general = (int64_t)f.n_general;
  b->direct_reach = (int32_t)std::max<uint32_t>(1u, std::max(f.max_l, f.max_span));
  b->direct_reach_ranges = b->direct_reach;
  // Chunks (a workgroup takes kDirectChunkTiles consecutive tiles and carries a tile's overhang on): position-sorted reads.  A
  // read that spans more than the overhang does not switch them off for the batch: the outliers are listed -- the ranges pass
  // then reaches back over the COMMON span only and direct_outliers_kernel adds them to the tiles they reach -- and only the
  // chunks they touch are dealt tile by tile.  Too many of them for the list (reads longer than the overhang, say): as before
  // round 6 -- the full reach, no chunks.
  b->direct_chunks = false;
  if (kDirectChunkTiles > 1 && f.unsorted == 0 && f.max_l <= (uint32_t)b->direct_overhang) {
    uint32_t listed = 0;
    HIP_TRY(ctx, hipMemcpy(&listed, b->d_n_outliers, 4, hipMemcpyDeviceToHost));
    if (listed <= b->outlier_cap) {
      b->direct_chunks = true;
      b->n_outliers_listed = listed;
      if (f.n_outliers > 0) {
        b->direct_reach_ranges = (int32_t)std::max<uint32_t>(1u, std::max(f.max_l, f.max_common));
        const int64_t n_chunked = (b->n_tiles - b->n_tiles / kDirectTailDiv) / kDirectChunkTiles * kDirectChunkTiles;
        std::vector<uint8_t> flag(nt), ok((size_t)std::max<int64_t>(1, n_chunked / kDirectChunkTiles), 1);
        HIP_TRY(ctx, hipMemcpy(flag.data(), b->d_tile_flag, nt, hipMemcpyDeviceToHost));
        for (int64_t t = 0; t < n_chunked; ++t)
          if (flag[(size_t)t]) ok[(size_t)(t / kDirectChunkTiles)] = 0;
        HIP_TRY(ctx, batch_alloc(b, &b->d_chunk_ok, ok.size()));
        HIP_TRY(ctx, hipMemcpy(b->d_chunk_ok, ok.data(), ok.size(), hipMemcpyHostToDevice));
      }
    }
  }
  b->alg_bytes = (int64_t)f.alg + 17 * b->n_sites;
  b->n_long = (int64_t)f.n_long;
  return MIDAS_SNPS_OK;
}

// step 3, a batch of the caller's arrays: the direct layout -- one 16-byte record per read and its CIGAR / SEQ / QUAL bytes as one
// run of the payload (every read was validated by the facts pass).  A resident batch has it already: the device decoder wrote it
// (bam_walk.hip, bam_direct_kernel).
int32_t build_layout(midas_snps_batch* b) {
  midas_snps_ctx* ctx = b->ctx;
  hipStream_t s = ctx->stream;
  const size_t n1 = (size_t)(b->n_reads > 0 ? b->n_reads : 1);
  const int nb = direct_index_blocks(b->n_reads);
  unsigned long long* d_units = nullptr;      // (scratch of the layout's scan + the layout's flags: the caller's columns stay, no side copies)
  HIP_TRY(ctx, batch_alloc(b, &b->d_drec, (n1 + 1) * sizeof(DirectRec)));
  HIP_TRY(ctx, hipMemsetAsync(b->d_drec, 0, (n1 + 1) * sizeof(DirectRec), s));
  HIP_TRY(ctx, batch_alloc(b, &d_units, ((size_t)nb + 1) * 8 + sizeof(DenseSide)));
  DenseSide* const d_side = reinterpret_cast<DenseSide*>(d_units + nb + 1);
  HIP_TRY(ctx, hipMemsetAsync(d_side, 0, sizeof(DenseSide), s));
  DirectLayoutParams lp;
  fill_raw_columns(b, &lp);
  lp.n_reads = b->n_reads;
  lp.block_units = d_units;
  lp.rec = b->d_drec;
  lp.payload = nullptr;
  lp.side = d_side;
  unsigned long long units = 0;
  hipEvent_t lev[2] = {nullptr, nullptr};       // (how long the layout takes on the device: reported beside the step it feeds)
  struct EvGuard { hipEvent_t* e; ~EvGuard() { for (int k = 0; k < 2; ++k) if (e[k]) (void)hipEventDestroy(e[k]); } } ev_guard{lev};
  HIP_TRY(ctx, hipEventCreate(&lev[0]));
  HIP_TRY(ctx, hipEventCreate(&lev[1]));
  HIP_TRY(ctx, hipEventRecord(lev[0], s));
  if (b->n_reads > 0) {
    HIP_TRY(ctx, launch_direct_layout_sizes(lp, s));
    HIP_TRY(ctx, hipMemcpyAsync(&units, d_units + nb, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
  }
  if (units > kMaxDirectPayloadUnits) {
    char buf[160];
    snprintf(buf, sizeof buf, "read payload of %llu bytes exceeds the 32 GiB a batch can address", units * 8ull);
    return fail(ctx, MIDAS_SNPS_ERR_UNSUPPORTED, buf);
  }
  const size_t payload_bytes = (size_t)(units * 8ull);
  constexpr size_t kPaySlack = 64;            // a lane's 16-byte loads may overhang the last read
  HIP_TRY(ctx, batch_alloc(b, &b->d_dpay, payload_bytes + kPaySlack));
  HIP_TRY(ctx, hipMemsetAsync(b->d_dpay + payload_bytes, 0, kPaySlack, s));
  lp.payload = b->d_dpay;
  if (b->n_reads > 0) HIP_TRY(ctx, launch_direct_layout_fill(lp, s));
  HIP_TRY(ctx, hipEventRecord(lev[1], s));
  DenseSide h_side{};
  HIP_TRY(ctx, hipMemcpyAsync(&h_side, d_side, sizeof h_side, hipMemcpyDeviceToHost, s));
  HIP_TRY(ctx, hipEventSynchronize(lev[1]));
  HIP_TRY(ctx, hipStreamSynchronize(s));
  b->dense_clamped = (h_side.flags & kDenseClampedQual) != 0u;
  float lms = 0.f;
  if (hipEventElapsedTime(&lms, lev[0], lev[1]) == hipSuccess) b->layout_build_us = (int32_t)(lms * 1000.f + 0.5f);
  (void)hipGetLastError();
  return MIDAS_SNPS_OK;
}

// One ranges pass on the batch's current parity, as every run of the direct path starts: the tile ranges from the positions, then
// the listed outliers added to the tiles they reach (when the ranges kept to the common span).  The caller advances
// direct_run_count once the pass's consumers are enqueued.
int32_t ranges_pass(midas_snps_batch* b, DirectIndexParams* ip) {
  midas_snps_ctx* ctx = b->ctx;
  hipStream_t s = ctx->stream;
  fill_direct_index(b, ip);
  HIP_TRY(ctx, launch_direct_ranges(*ip, s));
  if (b->direct_reach_ranges != b->direct_reach) HIP_TRY(ctx, launch_direct_outliers(b->d_outliers, b->n_outliers_listed, ip->tbegin, s));
  return MIDAS_SNPS_OK;
}

// step 4: the tile ranges once, to see how well the reads are ordered -- a tile's stream holds every read between the first and
// the last that can touch it -- and the path the batch's own numbers recommend
int32_t probe_ranges_and_choose(midas_snps_batch* b) {
  midas_snps_ctx* ctx = b->ctx;
  hipStream_t s = ctx->stream;
  const size_t nt = (size_t)(b->n_tiles > 0 ? b->n_tiles : 1);
  DirectIndexParams ip;
  ST_TRY(ranges_pass(b, &ip));
  std::vector<uint32_t> tb(nt), te(nt);
  HIP_TRY(ctx, hipMemcpyAsync(tb.data(), ip.tbegin, nt * 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(ctx, hipMemcpyAsync(te.data(), ip.tend, nt * 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(ctx, hipStreamSynchronize(s));
  b->direct_run_count += 1;
  int64_t stream = 0, worst = 0;
  for (size_t k = 0; k < (size_t)b->n_tiles; ++k) {
    const int64_t n0 = te[k] > tb[k] ? (int64_t)te[k] - (int64_t)tb[k] : 0;
    stream += n0;
    worst = std::max(worst, n0);
  }
  b->direct_stream_reads = stream;
  b->direct_max_tile_reads = worst;
  // Coordinate-sorted input makes the streams add up to the reads plus the few that straddle a tile border.  Much more than
  // that (unsorted input, or one read with a reference span of many tiles), or one tile holding far more than a workgroup's
  // fair share (a coverage hot spot: the packed path cuts such a tile into parts), and the packed path is the faster one.
  const int64_t fair = stream / (kWorkgroupsPerCU * (int64_t)ctx->prop.multiProcessorCount) + 1;
  const bool ordered = stream <= b->n_reads + b->n_reads / 2 + 4096;
  const bool hot = worst > std::max<int64_t>(2048, 2 * fair);
  b->path_auto = (ordered && !hot) ? MIDAS_SNPS_PATH_DIRECT : MIDAS_SNPS_PATH_PACKED;
  b->path = ctx->default_path == MIDAS_SNPS_PATH_AUTO ? b->path_auto : ctx->default_path;
  return MIDAS_SNPS_OK;
}

}  // namespace

// Buffers of the direct path, its facts pass (once: every read validated on the device -- the statuses of the packer --, the
// batch's totals, the longest reference span of a read) and one ranges pass: the numbers the choice of path rests on.
int32_t midas_batch::direct_prepare(midas_snps_batch* b) {
  ST_TRY(allocate_and_reset(b));
  ST_TRY(facts_and_summary(b));
  if (b->n_long > 0) {      // a read beyond the fast paths' limits: the whole batch takes the long path, nothing else is built
    b->path_auto = b->path = MIDAS_SNPS_PATH_LONG;
    return MIDAS_SNPS_OK;
  }
  b->direct_lane_bases = direct_lane_bases(b->max_l_seq);
  b->direct_lanes_per_read = b->max_l_seq <= b->direct_lane_bases ? 1 : (b->max_l_seq + b->direct_lane_bases - 1) / b->direct_lane_bases;
  if (b->resident) b->dense_clamped = (b->rr.dense_flags & kDenseClampedQual) != 0u;      // (the handle's flag: the whole file's reads, not just this batch's)
  else ST_TRY(build_layout(b));
  ST_TRY(probe_ranges_and_choose(b));
#if MIDAS_SNPS_DEBUG_BITS & 256
  midas_snps_ctx* ctx = b->ctx;
  HIP_TRY(ctx, batch_alloc(b, &b->d_probe, (size_t)ctx->prop.multiProcessorCount * kWorkgroupsPerCU * (kPileupBlock / 64) * 8 * 8));
  HIP_TRY(ctx, hipMemset(b->d_probe, 0, (size_t)ctx->prop.multiProcessorCount * kWorkgroupsPerCU * (kPileupBlock / 64) * 8 * 8));
#endif
  return MIDAS_SNPS_OK;
}

// A run on the direct path: the tile ranges from the positions, then the pileup kernel over the direct layout (one visit per read).
int32_t midas_batch::run_direct(midas_snps_batch* b, const midas_snps_thresholds* thr, hipEvent_t* ev) {
  midas_snps_ctx* ctx = b->ctx;
  hipStream_t s = ctx->stream;
  DirectIndexParams dip;
  ST_TRY(ranges_pass(b, &dip));
  if (ev) HIP_TRY(ctx, hipEventRecord(ev[1], s));
  DirectParams dp;
  dp.rec = b->d_drec; dp.payload = b->d_dpay;
  dp.tbegin = dip.tbegin; dp.tend = dip.tend;
  dp.probe = b->d_probe;
  dp.ref = b->d_ref;
  dp.tiles = b->d_tiles;
  dp.filt = b->d_filt;
  dp.out_counts = b->d_counts; dp.out_allele = b->d_allele;
  dp.stats = work_stats(b); dp.err = work_err(b);
  dp.sched = b->d_ticket + b->n_tiles;
  dp.n_tiles = (int32_t)b->n_tiles; dp.n_reads = (int32_t)b->n_reads;
  const bool chunks = b->direct_chunks && (b->direct_overhang == kDirectOverhang || b->filt_fits16);
  dp.overhang = chunks ? b->direct_overhang : kDirectOverhang;      // (no chunks: nothing is carried, the common instantiation)
  dp.grid_blocks = ctx->prop.multiProcessorCount * kWorkgroupsPerCU;      // (the long overhang's instantiation keeps its tables in 16 bits: four workgroups a CU as well)
#ifdef MIDAS_SNPS_GRID_BLOCKS
  dp.grid_blocks = MIDAS_SNPS_GRID_BLOCKS;
#endif
  dp.lanes_per_read = b->direct_lanes_per_read;
  dp.reads_per_wave = 64 / b->direct_lanes_per_read;
  dp.table_len = b->max_l_seq + 1;
  dp.baseq = thr->baseq; dp.mapq_min = thr->mapq; dp.readq = thr->readq;
  dp.pad_advances = b->pad_advances ? 1 : 0;
  // chunks of consecutive tiles with a carried overhang (a read visited once): position-sorted reads none of which spans more
  // than the overhang; the last eighth of the tiles one by one, so that the workgroups finish together
  dp.chunk_tiles = 1; dp.n_chunked_tiles = 0;
  dp.chunk_ok = b->d_chunk_ok;
  if (chunks) {
    dp.chunk_tiles = kDirectChunkTiles;
    dp.n_chunked_tiles = (int32_t)((b->n_tiles - b->n_tiles / kDirectTailDiv) / kDirectChunkTiles * kDirectChunkTiles);
  }
  HIP_TRY(ctx, launch_pileup_direct(dp, b->direct_lane_bases, s));
  b->direct_run_count += 1;
  return MIDAS_SNPS_OK;
}

extern "C" {

// Test aid (tests/test_gpu_index.py): the ranges pass of a run -- ranges_pass, not a copy of it -- on the current parity, then the
// ranges, the facts and what the batch derived from them, the outlier list, the tile flags and chunk_ok on the host.
int32_t midas_snps_batch_fetch_index(midas_snps_batch* b, uint32_t* tbegin, uint32_t* tend, int64_t* facts, uint32_t* outliers3, uint8_t* tile_flag,
                                     uint8_t* chunk_ok, int64_t* out_n_chunk_ok) {
  if (!b || (chunk_ok && !out_n_chunk_ok)) return MIDAS_SNPS_ERR_INVALID_ARG;
  midas_snps_ctx* ctx = b->ctx;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (b->n_long > 0 || !b->d_trange) return fail(ctx, MIDAS_SNPS_ERR_UNSUPPORTED, "the batch has the long path only: no tile ranges were built");
  hipStream_t s = ctx->stream;
  DirectIndexParams ip;
  ST_TRY(ranges_pass(b, &ip));
  b->direct_run_count += 1;
  const size_t nt = (size_t)b->n_tiles;
  if (tbegin && nt) HIP_TRY(ctx, hipMemcpyAsync(tbegin, ip.tbegin, nt * 4, hipMemcpyDeviceToHost, s));
  if (tend && nt) HIP_TRY(ctx, hipMemcpyAsync(tend, ip.tend, nt * 4, hipMemcpyDeviceToHost, s));
  if (tile_flag && nt) HIP_TRY(ctx, hipMemcpyAsync(tile_flag, b->d_tile_flag, nt, hipMemcpyDeviceToHost, s));
  const uint32_t n_out = std::min(b->n_outliers_listed, b->outlier_cap);
  std::vector<DirectOutlier> list(outliers3 ? n_out : 0u);
  if (!list.empty()) HIP_TRY(ctx, hipMemcpyAsync(list.data(), b->d_outliers, list.size() * sizeof(DirectOutlier), hipMemcpyDeviceToHost, s));
  const int64_t n_ok = b->d_chunk_ok ? std::max<int64_t>(1, (b->n_tiles - b->n_tiles / kDirectTailDiv) / kDirectChunkTiles) : 0;
  if (chunk_ok && n_ok) HIP_TRY(ctx, hipMemcpyAsync(chunk_ok, b->d_chunk_ok, (size_t)n_ok, hipMemcpyDeviceToHost, s));
  HIP_TRY(ctx, hipStreamSynchronize(s));
  for (size_t k = 0; k < list.size(); ++k) {
    outliers3[3 * k] = list[k].read; outliers3[3 * k + 1] = list[k].t_first; outliers3[3 * k + 2] = list[k].t_last;
  }
  if (out_n_chunk_ok) *out_n_chunk_ok = n_ok;
  if (facts) {
    const DirectFactsSum& f = b->direct_facts;
    const int64_t v[MIDAS_SNPS_INDEX_FACTS] = {
        (int64_t)f.status, (int64_t)f.alg, (int64_t)f.n_general, (int64_t)f.n_long, (int64_t)f.n_outliers, f.max_l, f.max_span, f.max_common,
        f.unsorted, b->direct_reach, b->direct_reach_ranges, b->direct_overhang, b->direct_chunks ? 1 : 0, b->n_outliers_listed, b->outlier_cap};
    std::copy(v, v + MIDAS_SNPS_INDEX_FACTS, facts);
  }
  return MIDAS_SNPS_OK;
}

}  // extern "C"
