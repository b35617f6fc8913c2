// The table writer of a batch (midas_snps_batch_write_part) and the row coder's host side: rows formatted and deflated on the
// device (rows_deflate.hip) or fed slab by slab to the host's formatter, straight from the batch's device results.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <mutex>
#include <vector>

#include "../../include/midas_snps.h"
#include "batch.h"

using namespace midas;
using namespace midas_ctx;

// Rows of a table straight from the batch's device results: the formatter's threads work on one slab of sites in the
// context's pinned ring while the next one crosses the link, so neither a host copy of the whole result nor the time of
// its transfer is ever paid on its own.
extern "C" {

namespace {
// The ring: the context's two 32 MiB staging buffers cut into 16 slots of 4 MiB (15 gzip members each).  Many small
// slabs, not two large ones: a slot is reused only when every member of its previous slab is done, so with two slabs of
// ~125 members each and ~128 formatter threads the whole pool moved in lock step at the pace of its slowest thread
// (measured on a shared host: three rounds of ~86 ms).  With 240 members in flight a straggler holds up nobody.
constexpr int kFeedSlotsPerStage = 8;
constexpr size_t kFeedSlotBytes = midas_snps_ctx::kStageBytes / kFeedSlotsPerStage;
struct BatchFeed {
  midas_snps_batch* b;
  int64_t slab_sites;
  hipError_t err = hipSuccess;
};
bool batch_feed_fetch(void* user, int slot, int64_t src_lo, int64_t n, const uint8_t** allele, const uint32_t** counts) {
  BatchFeed* f = static_cast<BatchFeed*>(user);
  midas_snps_batch* b = f->b;
  midas_snps_ctx* ctx = b->ctx;
  hipStream_t s = ctx->stream;
  hipError_t e = hipSetDevice(ctx->device);     // (called from one of the library's worker threads)
  uint8_t* base = static_cast<uint8_t*>(ctx->stage[slot / kFeedSlotsPerStage]) + (size_t)(slot % kFeedSlotsPerStage) * kFeedSlotBytes;
  uint8_t* al = base + (size_t)f->slab_sites * 16;
  if (e == hipSuccess && n > 0) {
    void* mapped = nullptr;
    if (hipHostGetDevicePointer(&mapped, base, 0) == hipSuccess && mapped) {
      e = launch_copy16(mapped, b->d_counts + 4 * src_lo, (size_t)n, 1024, s);
    } else {
      (void)hipGetLastError();
      e = hipMemcpyAsync(base, b->d_counts + 4 * src_lo, (size_t)n * 16, hipMemcpyDeviceToHost, s);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(al, b->d_allele + src_lo, (size_t)n, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
  }
  if (e != hipSuccess) { f->err = e; return false; }
  *allele = al;
  *counts = reinterpret_cast<const uint32_t*>(base);
  return true;
}
// The arena a launch of the row kernel gets: the tables of a 20x genome take ~4 bytes a row; ten a row and a header's worth per
// member is room for any coverage seen so far, and a member that does not fit sends the part to the host's formatter.
unsigned long long rows_arena_rule(int64_t rows, int64_t n_members) {
  return (unsigned long long)rows * 10ull + (unsigned long long)n_members * 1024ull + 4096ull;
}

// What one launch of the row kernel leaves behind.
struct CodedRows {
  std::vector<RowsResult> results;     // one per member, in the members' order
  unsigned long long used = 0;         // the arena's cursor after the launch (beyond arena_bytes when a member did not fit)
  uint8_t* streams = nullptr;          // the arena's first min(used, arena_bytes) bytes: a member's stream is at its result's off
  bool all_coded = false;              // every member came back with status 0
  ~CodedRows() { free(streams); }      // (malloc: no zero fill)
};

// The device half of the row coder (rows_deflate.hip), the one launch behind midas_snps_batch_write_part and midas_snps_rows_code:
// members and ids up, arena and cursor zeroed, the kernel over `grid_blocks` workgroups, results and streams down.  The members go to
// the kernel as they are.  The streams of a launch in which some member was declined are copied only when `keep_declined` says so
// (the table writer leaves such a part to the host's formatter and has no use for them).
// Several host threads write one table each.  What they share is taken in turn, and as briefly as it can be: the context's
// stream for the row kernel (device_mutex), then the pinned ring + the copy stream for the streams' way down (copy_mutex) --
// table k's bytes cross the link while table k + 1 is formatted and deflated.  The allocations are nobody's turn.
int32_t code_rows_on_device(midas_snps_ctx* ctx, const uint32_t* d_counts, const uint8_t* d_allele, const std::vector<RowsMember>& members,
                            const std::vector<uint8_t>& ids, unsigned long long arena_bytes, int grid_blocks, bool keep_declined,
                            CodedRows* out, const std::function<void(const char*)>& lap) {
  const int64_t n_members = (int64_t)members.size();
  out->results.assign((size_t)n_members, RowsResult{});
  HIP_TRY(ctx, hipSetDevice(ctx->device));       // (the calling thread may never have talked to the device)
  struct PooledBuf {      // one buffer (the context keeps a few between tables): | arena | members | results | cursor | ids |
    midas_snps_ctx* ctx; void* p = nullptr; size_t bytes = 0;
    ~PooledBuf() { if (p) ctx->row_buffers.give(p, bytes); }
  } d_arena{ctx};
  auto up256 = [](size_t v) { return (v + 255) & ~(size_t)255; };
  const size_t at_members = up256((size_t)arena_bytes), at_results = at_members + up256((size_t)n_members * sizeof(RowsMember)),
               at_cursor = at_results + up256((size_t)n_members * sizeof(RowsResult)), at_ids = at_cursor + 256;
  d_arena.p = ctx->row_buffers.take(at_ids + ids.size() + 16, &d_arena.bytes);
  if (!d_arena.p) return fail(ctx, MIDAS_SNPS_ERR_OUT_OF_MEMORY, "row coder: out of device memory for a table's coded rows");
  uint8_t* const d_base = static_cast<uint8_t*>(d_arena.p);
  struct Part { void* p; } d_members{d_base + at_members}, d_results{d_base + at_results}, d_cursor{d_base + at_cursor}, d_ids{d_base + at_ids};
  lap("members + hipMalloc");
  {
  std::lock_guard<std::mutex> device_part(ctx->device_mutex);
  hipStream_t s = ctx->stream;
  HIP_TRY(ctx, hipMemcpyAsync(d_members.p, members.data(), (size_t)n_members * sizeof(RowsMember), hipMemcpyHostToDevice, s));
  if (!ids.empty()) HIP_TRY(ctx, hipMemcpyAsync(d_ids.p, ids.data(), ids.size(), hipMemcpyHostToDevice, s));
  HIP_TRY(ctx, hipMemsetAsync(d_arena.p, 0, (size_t)arena_bytes, s));
  HIP_TRY(ctx, hipMemsetAsync(d_cursor.p, 0, 8, s));
  RowsParams rp;
  rp.counts = d_counts; rp.allele = d_allele;
  rp.ids = static_cast<const uint8_t*>(d_ids.p);
  rp.members = static_cast<const RowsMember*>(d_members.p);
  rp.n_members = (int32_t)n_members;
  rp.arena = static_cast<uint8_t*>(d_arena.p); rp.arena_bytes = arena_bytes;
  rp.cursor = static_cast<unsigned long long*>(d_cursor.p);
  rp.results = static_cast<RowsResult*>(d_results.p);
  HIP_TRY(ctx, launch_rows_deflate(rp, grid_blocks, s));
  HIP_TRY(ctx, hipMemcpyAsync(out->results.data(), d_results.p, (size_t)n_members * sizeof(RowsResult), hipMemcpyDeviceToHost, s));
  HIP_TRY(ctx, hipMemcpyAsync(&out->used, d_cursor.p, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(ctx, hipStreamSynchronize(s));
  lap("its turn, memset + kernel");
  }
  out->all_coded = out->used <= arena_bytes;
  for (const RowsResult& r : out->results)
    if (r.status != 0u) out->all_coded = false;
  if (!out->all_coded && !keep_declined) return MIDAS_SNPS_OK;
  const size_t down = (size_t)std::min(out->used, arena_bytes);
  out->streams = static_cast<uint8_t*>(malloc(down + 16));
  if (!out->streams) return fail(ctx, MIDAS_SNPS_ERR_OUT_OF_MEMORY, "row coder: out of host memory");
  {
    hipStream_t cs = nullptr;
    {
      std::lock_guard<std::mutex> g(ctx->copy_mutex);
      if (!ctx->copy_stream && hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); ctx->copy_stream = nullptr; }
      cs = ctx->copy_stream;
    }
    // (the row kernel is over -- the stream was waited for above: the copy depends on nothing that is still running)
    ST_TRY(copy_to_host(ctx, out->streams, d_arena.p, down, cs));
  }
  lap("streams to host");
  return MIDAS_SNPS_OK;      // (the device buffer goes back to the context here, before the caller writes its file: the next table takes it)
}

// The rows of the given contigs formatted and deflated on the device (rows_deflate.hip), framed and written by the host.
// Returns MIDAS_SNPS_OK with *done = false when the device coder declines a member (a contig id beyond its limit, an arena
// that turned out too small): the caller then takes the host's formatter for the whole part.
int32_t write_part_on_device(midas_snps_batch* b, const char* path, bool with_header, int32_t n_contigs, const int64_t* src,
                             const int64_t* n_sites, const int64_t* first, const char* const* ref_ids, int32_t gz_level,
                             int32_t threads, bool* done) {
  midas_snps_ctx* ctx = b->ctx;
  *done = false;
  // MIDAS_SNPS_TRACE=1: where the call spends its time, on stderr
  const bool trace = getenv("MIDAS_SNPS_TRACE") != nullptr;
  auto now = [] { return std::chrono::steady_clock::now(); };
  auto t_last = now();
  auto lap = [&](const char* what) {
    if (!trace) return;
    const auto t = now();
    fprintf(stderr, "[rows on device] %-28s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(t - t_last).count());
    t_last = t;
  };
  std::vector<RowsMember> members;
  std::vector<uint8_t> ids;
  for (int32_t k = 0; k < n_contigs; ++k) {
    const size_t id_off = ids.size(), id_len = strlen(ref_ids[k]);
    if (id_len > 192) { ctx->rows_parts_declined_id += 1; return MIDAS_SNPS_OK; }
    ids.insert(ids.end(), ref_ids[k], ref_ids[k] + id_len);
    for (int64_t lo = 0; lo < n_sites[k]; lo += kRowsPerMember) {
      RowsMember m;
      m.site0 = src[k] + lo;
      m.pos0 = first[k] + lo + 1;
      m.n_rows = (int32_t)std::min<int64_t>(kRowsPerMember, n_sites[k] - lo);
      m.id_off = (int32_t)id_off; m.id_len = (int32_t)id_len; m.pad = 0;
      members.push_back(m);
    }
  }
  const int64_t n_members = (int64_t)members.size();
  char err[256] = {0};
  if (n_members == 0) {
    const int32_t st = write_coded_members(path, with_header, gz_level, 0, nullptr, threads, err);
    if (st != MIDAS_SNPS_OK) return fail(ctx, st, err);
    *done = true;
    return MIDAS_SNPS_OK;
  }
  if (n_members > 0x7FFFFFFFll || ids.size() > 0x7FFFFFFFull) return MIDAS_SNPS_OK;
  int64_t rows = 0;
  for (const RowsMember& m : members) rows += m.n_rows;
  CodedRows coded_rows;
  ST_TRY(code_rows_on_device(ctx, b->d_counts, b->d_allele, members, ids, rows_arena_rule(rows, n_members), ctx->prop.multiProcessorCount, false,
                             &coded_rows, lap));
  if (!coded_rows.all_coded) { ctx->rows_parts_declined_status += 1; return MIDAS_SNPS_OK; }
  std::vector<CodedMember> coded((size_t)n_members);
  for (int64_t k = 0; k < n_members; ++k) {
    const RowsResult& r = coded_rows.results[(size_t)k];
    coded[(size_t)k] = CodedMember{coded_rows.streams + r.off, r.n_bytes, r.crc, r.text_len, (uint32_t)members[(size_t)k].n_rows};
  }
  const int32_t st = write_coded_members(path, with_header, gz_level, n_members, coded.data(), threads, err);
  if (st != MIDAS_SNPS_OK) {
    std::lock_guard<std::mutex> g(ctx->device_mutex);
    return fail(ctx, st, err);
  }
  lap("frame + write");
  ctx->rows_members_on_device += n_members;
  *done = true;
  return MIDAS_SNPS_OK;
}
}  // namespace

int32_t midas_snps_row_coder_counts(const midas_snps_ctx* ctx, int64_t out3[3]) {
  if (!ctx || !out3) return MIDAS_SNPS_ERR_INVALID_ARG;
  out3[0] = ctx->rows_members_on_device.load();
  out3[1] = ctx->rows_parts_declined_id.load();
  out3[2] = ctx->rows_parts_declined_status.load();
  return MIDAS_SNPS_OK;
}

int32_t midas_snps_rows_code(midas_snps_ctx* ctx, int64_t n_sites, const uint32_t* counts, const uint8_t* allele, int32_t n_members,
                             const int64_t* site0, const int64_t* pos0, const int32_t* n_rows, const int32_t* id_off, const int32_t* id_len,
                             const uint8_t* ids, int64_t ids_bytes, int64_t arena_bytes, int32_t grid_blocks, uint32_t* out_status,
                             uint32_t* out_n_bytes, uint32_t* out_crc, uint32_t* out_text_len, int64_t* out_arena_off, uint8_t* out_streams,
                             int64_t out_cap, int64_t* out_stream_bytes) {
  if (!ctx || n_sites <= 0 || !counts || !allele || n_members <= 0 || !site0 || !pos0 || !n_rows || !id_off || !id_len || ids_bytes < 0 ||
      (ids_bytes > 0 && !ids) || arena_bytes < 0 || grid_blocks < 0 || !out_status || !out_n_bytes || !out_crc || !out_text_len ||
      !out_arena_off || out_cap < 0 || (out_cap > 0 && !out_streams) || !out_stream_bytes)
    return MIDAS_SNPS_ERR_INVALID_ARG;
  // the kernel takes the members as they are; what is checked here is only that a member it WILL take (1..16 384 rows, an id within
  // its limit) reads nothing outside the arrays it was given and numbers its rows below 2^31
  std::vector<RowsMember> members((size_t)n_members);
  int64_t rows = 0;
  for (int32_t k = 0; k < n_members; ++k) {
    if (id_len[k] < 0 || id_off[k] < 0 || (int64_t)id_off[k] + id_len[k] > ids_bytes)
      return fail(ctx, MIDAS_SNPS_ERR_INVALID_ARG, "rows_code: a member's id lies outside the ids");
    if (n_rows[k] > 0 && n_rows[k] <= kRowsPerMember &&
        (site0[k] < 0 || site0[k] + n_rows[k] > n_sites || pos0[k] < 0 || pos0[k] + n_rows[k] - 1 > 0x7FFFFFFFll))
      return fail(ctx, MIDAS_SNPS_ERR_INVALID_ARG, "rows_code: a member's sites or positions are out of range");
    RowsMember& m = members[(size_t)k];
    m.site0 = site0[k]; m.pos0 = pos0[k]; m.n_rows = n_rows[k]; m.id_off = id_off[k]; m.id_len = id_len[k]; m.pad = 0;
    rows += std::min<int64_t>(std::max<int64_t>(n_rows[k], 0), kRowsPerMember);
  }
  const std::vector<uint8_t> id_bytes(ids, ids + ids_bytes);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  DeviceBuf d_counts, d_allele;
  HIP_TRY(ctx, hipMalloc(&d_counts.p, (size_t)n_sites * 16));
  HIP_TRY(ctx, hipMalloc(&d_allele.p, (size_t)n_sites));
  {
    std::lock_guard<std::mutex> g(ctx->device_mutex);
    HIP_TRY(ctx, hipMemcpyAsync(d_counts.p, counts, (size_t)n_sites * 16, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(d_allele.p, allele, (size_t)n_sites, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  }
  CodedRows coded;
  ST_TRY(code_rows_on_device(ctx, static_cast<const uint32_t*>(d_counts.p), static_cast<const uint8_t*>(d_allele.p), members, id_bytes,
                             arena_bytes ? (unsigned long long)arena_bytes : rows_arena_rule(rows, n_members),
                             grid_blocks ? grid_blocks : ctx->prop.multiProcessorCount, true, &coded, [](const char*) {}));
  int64_t at = 0;
  for (int32_t k = 0; k < n_members; ++k) {
    const RowsResult& r = coded.results[(size_t)k];
    out_status[k] = r.status; out_n_bytes[k] = r.n_bytes; out_crc[k] = r.crc; out_text_len[k] = r.text_len;
    out_arena_off[k] = r.status == 0u ? (int64_t)r.off : -1;
    if (r.status != 0u) continue;
    if (at + (int64_t)r.n_bytes > out_cap) return fail(ctx, MIDAS_SNPS_ERR_INVALID_ARG, "rows_code: out_streams is too small for the streams");
    memcpy(out_streams + at, coded.streams + r.off, r.n_bytes);
    at += (int64_t)r.n_bytes;
  }
  *out_stream_bytes = at;
  return MIDAS_SNPS_OK;
}

int32_t midas_snps_batch_write_part(midas_snps_batch* b, const char* path, int32_t with_header, int32_t n_contigs,
                                    const int32_t* contig_index, const char* const* ref_ids, int32_t gz_level, int32_t threads) {
  if (!b || !path || n_contigs < 0 || (n_contigs > 0 && (!contig_index || !ref_ids))) return MIDAS_SNPS_ERR_INVALID_ARG;
  midas_snps_ctx* ctx = b->ctx;
  int32_t st;
  {   // (several host threads may be writing one table each: see ctx_internal.h, device_mutex)
    std::lock_guard<std::mutex> g(ctx->device_mutex);
    st = midas_snps_batch_sync(b);
    if (st != MIDAS_SNPS_OK) return st;
    if (!b->ran) return fail(ctx, MIDAS_SNPS_ERR_INVALID_ARG, "batch_write_part before batch_run");
  }
  std::vector<int64_t> n_sites((size_t)n_contigs), src((size_t)n_contigs), first((size_t)n_contigs, 0);
  for (int32_t k = 0; k < n_contigs; ++k) {
    const int32_t c = contig_index[k];
    if (c < 0 || c >= b->n_contigs || !ref_ids[k]) return fail(ctx, MIDAS_SNPS_ERR_INVALID_ARG, "batch_write_part: contig index out of range");
    src[(size_t)k] = b->h_contig_site[(size_t)c];
    n_sites[(size_t)k] = b->h_contig_site[(size_t)c + 1] - b->h_contig_site[(size_t)c];
    if (!b->h_origin.empty()) first[(size_t)k] = b->h_origin[(size_t)c];     // a piece's rows carry the contig's positions
  }
  // gz levels 1-5 are the row coder's: it runs on the device unless the context was told otherwise
  if (gz_level >= 1 && gz_level <= 5 && ctx->row_coder == MIDAS_SNPS_ROWS_DEVICE) {
    bool done = false;
    st = write_part_on_device(b, path, with_header != 0, n_contigs, src.data(), n_sites.data(), first.data(), ref_ids, gz_level,
                              threads, &done);
    if (st != MIDAS_SNPS_OK || done) return st;
  }
  std::lock_guard<std::mutex> host_path(ctx->device_mutex);      // (the host's formatter owns the staging ring for the whole call)
  std::lock_guard<std::mutex> host_ring(ctx->copy_mutex);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  constexpr size_t kChunk = midas_snps_ctx::kStageBytes;
  ctx->stage_join();
  for (int k = 0; k < midas_snps_ctx::kStageSlots; ++k)
    if (!ctx->stage[k]) HIP_TRY(ctx, hipHostMalloc(&ctx->stage[k], kChunk, kHostAllocFlags));
  BatchFeed user{b, (int64_t)(kFeedSlotBytes / 17 / (size_t)kRowsPerMember) * kRowsPerMember};
  RowFeed feed{src.data(), user.slab_sites, midas_snps_ctx::kStageSlots * kFeedSlotsPerStage, &user, batch_feed_fetch};
  char err[256] = {0};
  st = write_rows_fed(path, with_header != 0, n_contigs, ref_ids, n_sites.data(), gz_level, threads, feed, err, first.data());
  if (user.err != hipSuccess) return hip_fail(ctx, user.err, "batch_write_part: results to host");
  if (st != MIDAS_SNPS_OK) return fail(ctx, st, err);
  return MIDAS_SNPS_OK;
}

}  // extern "C"
