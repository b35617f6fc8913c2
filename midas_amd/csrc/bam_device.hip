// The device BAM decode behind the C ABI: the inflater on its own (midas_snps_inflate_blocks, midas_bam_open_device), the one-arena
// decode (device_decode_run) and the streamed decode (device_decode_stream), and the midas_bam_* entry points built from them.
// The steps the three share -- block tables, the second inflate pass, the record walk's tables, the columns -- are here once each;
// their host arithmetic (the arena's layout, the streamed decode's groups, the stitching of the walk's chunks) is decode_plan.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/midas_snps.h"
#include "ctx_internal.h"
#include "kernels.h"
#include "layout.h"
#include "hostio.h"
#include "decode_plan.h"

using namespace midas;
using namespace midas_ctx;

static_assert(sizeof(InflateBlock) == kInflateBlockBytes, "decode_plan.h lays out the block tables");

namespace {

// ---- errors and traces ----------------------------------------------------------------------------------------------------------
constexpr char kInflate[] = "device inflate", kDecode[] = "device decode", kStreamed[] = "device decode (streamed)",
               kToColumns[] = "resident BAM to columns", kGenes[] = "genes count over a BAM";
int32_t hip_err(char* err256, const char* who, hipError_t e, const char* what) {
  if (err256) snprintf(err256, 256, "%s: %s: %s", who, what, hipGetErrorString(e));
  (void)hipGetLastError();
  return e == hipErrorOutOfMemory ? MIDAS_SNPS_ERR_OUT_OF_MEMORY : MIDAS_SNPS_ERR_HIP;
}
// (in a function that has `err256`)
#define TRY(who, call) do { const hipError_t e__ = (call); if (e__ != hipSuccess) return hip_err(err256, who, e__, #call); } while (0)

// MIDAS_SNPS_TRACE: where a call spends its time, on stderr
using Clock = std::chrono::steady_clock;
double ms_since(Clock::time_point t) { return std::chrono::duration<double, std::milli>(Clock::now() - t).count(); }
struct Lap {
  const char* tag;
  int width;
  const bool on = getenv("MIDAS_SNPS_TRACE") != nullptr;
  Clock::time_point last = Clock::now();
  double take() {       // milliseconds since the last lap
    const double ms = ms_since(last);
    last = Clock::now();
    return ms;
  }
  void operator()(const char* what) {
    if (on) fprintf(stderr, "[%s] %-*s %8.3f ms\n", tag, width, what, take());
  }
};

struct Loan { std::shared_ptr<midas_arena_pool> pool; void* p; ~Loan() { if (p) pool->give(p); } };      // the context's arena, given back on every way out

// A region handed out piece by piece, every piece rounded up to 256 bytes; nullptr once a piece does not fit (and for every one after it)
struct Scratch {
  uint8_t* p;
  size_t bytes, at = 0;
  uint8_t* take(size_t n) { uint8_t* q = p + at; at += round256(n); return at <= bytes ? q : nullptr; }
  template <class T> T* as(size_t n) { return reinterpret_cast<T*>(take(n)); }
};

// ---- the inflate's steps ------------------------------------------------------------------------------------------------------
// The block table of jobs[0, n): a block's compressed bytes at c_at + (cpos - c0) of the device's copy, its inflated bytes at
// upos - u0, its match room behind *room (which moves on); want[k]: the CRC-32 its bytes must have.
void fill_inflate_blocks(const InflateJob* jobs, size_t n, uint64_t c0, uint64_t c_at, uint64_t u0, InflateBlock* blocks, uint32_t* want,
                         unsigned long long* room) {
  for (size_t k = 0; k < n; ++k) {
    const InflateJob& q = jobs[k];
    const uint32_t cap = first_pass_room(q.ulen);
    blocks[k] = InflateBlock{(unsigned long long)(c_at + (q.cpos - c0)), (unsigned long long)(q.upos - u0), *room, q.clen, q.ulen, cap, 0u};
    want[k] = q.crc;
    *room += cap;
  }
}

InflateParams inflate_params(const InflateLayout& L, uint8_t* base, size_t n) {
  InflateParams ip;
  ip.comp = base + L.at_comp;
  ip.blocks = reinterpret_cast<const InflateBlock*>(base + L.at_blocks);
  ip.n_blocks = (long long)n;
  ip.out = base;
  ip.status = reinterpret_cast<uint32_t*>(base + L.at_status);
  ip.n_matches = reinterpret_cast<uint32_t*>(base + L.at_status) + n;
  ip.matches = reinterpret_cast<unsigned long long*>(base + L.at_matches);
  ip.want_crc = reinterpret_cast<const uint32_t*>(base + L.at_crc);
  return ip;
}

}  // namespace

// The streams whose matches did not fit their room (status kInflateMatchRoom): again, with the bound's room, into the same output;
// their statuses replace the first pass's.  want: the streams' CRC-32 (nullptr: not checked).  (Shared with tables_device.hip.)
int32_t midas_ctx::inflate_again(const char* who, const InflateParams& ip, const InflateBlock* blocks, const uint32_t* want, std::vector<uint32_t>& status, hipStream_t s,
                      bool* ran, char* err256) {
  *ran = false;
  std::vector<size_t> again;
  for (size_t k = 0; k < status.size(); ++k)
    if (status[k] == kInflateMatchRoom) again.push_back(k);
  if (again.empty()) return MIDAS_SNPS_OK;
  *ran = true;
  const size_t n2 = again.size();
  std::vector<InflateBlock> b2(n2);
  std::vector<uint32_t> want2(n2);
  unsigned long long room2 = 0;
  for (size_t j = 0; j < n2; ++j) {
    const InflateBlock& q = blocks[again[j]];
    const uint32_t cap = second_pass_room(q.ulen);
    b2[j] = InflateBlock{q.cpos, q.upos, room2, q.clen, q.ulen, cap, 0u};
    if (want) want2[j] = want[again[j]];
    room2 += cap;
  }
  DeviceBuf d_b2, d_s2, d_m2, d_c2;
  TRY(who, hipMalloc(&d_b2.p, n2 * sizeof(InflateBlock)));
  TRY(who, hipMalloc(&d_s2.p, n2 * 8));
  TRY(who, hipMalloc(&d_m2.p, (size_t)room2 * 8));
  TRY(who, hipMemcpyAsync(d_b2.p, b2.data(), n2 * sizeof(InflateBlock), hipMemcpyHostToDevice, s));
  if (want) {
    TRY(who, hipMalloc(&d_c2.p, n2 * 4));
    TRY(who, hipMemcpyAsync(d_c2.p, want2.data(), n2 * 4, hipMemcpyHostToDevice, s));
  }
  InflateParams ip2 = ip;
  ip2.blocks = static_cast<const InflateBlock*>(d_b2.p);
  ip2.n_blocks = (long long)n2;
  ip2.status = static_cast<uint32_t*>(d_s2.p);
  ip2.n_matches = static_cast<uint32_t*>(d_s2.p) + n2;
  ip2.matches = static_cast<unsigned long long*>(d_m2.p);
  ip2.want_crc = static_cast<const uint32_t*>(d_c2.p);
  TRY(who, launch_bgzf_inflate(ip2, s));
  std::vector<uint32_t> st2(n2);
  TRY(who, hipMemcpyAsync(st2.data(), d_s2.p, n2 * 4, hipMemcpyDeviceToHost, s));
  TRY(who, hipStreamSynchronize(s));
  for (size_t j = 0; j < n2; ++j) status[again[j]] = st2[j];
  return MIDAS_SNPS_OK;
}

namespace {

// the first block of a decode that did not inflate to its bytes: named by its index in the file's table (job0: the first status's)
int32_t check_block_statuses(const std::vector<uint32_t>& status, size_t job0, int64_t* bad_job, char* err256) {
  for (size_t k = 0; k < status.size(); ++k) {
    if (status[k] != 0u) {
      *bad_job = (int64_t)(job0 + k);
      if (err256) snprintf(err256, 256, "corrupt BGZF block %lld (code %u)", (long long)(job0 + k), status[k]);
      return MIDAS_SNPS_ERR_BAD_LAYOUT;
    }
  }
  return MIDAS_SNPS_OK;
}

// midas::BlockInflater over a context: the streams go to the device, one thread inflates each (bgzf_inflate.hip), the
// inflated bytes come back through the staging ring.
struct InflateUser {
  midas_snps_ctx* ctx;
  bool keep = false;            // leave the inflated stream on the device: `kept` (the caller frees it)
  void* kept = nullptr;         // the arena; the inflated stream is at its start
  size_t kept_bytes = 0;
  uint8_t* scratch = nullptr;   // what lies behind the stream in the arena: dead once the call returns, the caller's to reuse
  size_t scratch_bytes = 0;
};
int32_t device_inflate(void* user, const InflateSegment* segs, size_t n_segs, const InflateJob* jobs, size_t n_jobs, uint8_t* out,
                       size_t out_bytes, int64_t* bad_job, char* err256) {
  InflateUser* iu = static_cast<InflateUser*>(user);
  midas_snps_ctx* ctx = iu->ctx;
  if (bad_job) *bad_job = -1;
  if (n_jobs == 0) return MIDAS_SNPS_OK;
  size_t comp_bytes = 0;
  for (size_t k = 0; k < n_segs; ++k) comp_bytes += segs[k].n;
  for (size_t k = 0; k < n_jobs; ++k) {
    if (jobs[k].cpos + jobs[k].clen > comp_bytes || jobs[k].upos + jobs[k].ulen > out_bytes) {
      if (err256) snprintf(err256, 256, "device inflate: stream %lld lies outside the buffers", (long long)k);
      return MIDAS_SNPS_ERR_INVALID_ARG;
    }
  }
  std::lock_guard<std::mutex> g(ctx->device_mutex);
  Lap lap{"device inflate", 24};
  TRY(kInflate, hipSetDevice(ctx->device));
  std::vector<InflateBlock> blocks(n_jobs);
  std::vector<uint32_t> want(n_jobs);
  unsigned long long n_match_room = 0;
  fill_inflate_blocks(jobs, n_jobs, 0, 0, 0, blocks.data(), want.data(), &n_match_room);
  bool check = true;       // the streams' CRC-32 is verified when every one of them brings it (BGZF blocks do)
  for (size_t k = 0; k < n_jobs; ++k) check = check && jobs[k].check_crc != 0u;
  const InflateLayout L(out_bytes, comp_bytes, n_jobs, (size_t)n_match_room);
  DeviceBuf arena;
  TRY(kInflate, hipMalloc(&arena.p, L.end));
  uint8_t* const base = static_cast<uint8_t*>(arena.p);
  InflateParams ip = inflate_params(L, base, n_jobs);
  if (!check) ip.want_crc = nullptr;
  hipStream_t s = ctx->stream;
  size_t at = 0;
  for (size_t k = 0; k < n_segs; ++k) {
    if (segs[k].n) TRY(kInflate, hipMemcpyAsync(base + L.at_comp + at, segs[k].p, segs[k].n, hipMemcpyHostToDevice, s));
    at += segs[k].n;
  }
  TRY(kInflate, hipMemsetAsync(base + L.at_comp + comp_bytes, 0, 512, s));
  if (lap.on) { TRY(kInflate, hipStreamSynchronize(s)); lap("hipMalloc + streams up"); }
  TRY(kInflate, hipMemcpyAsync(base + L.at_blocks, blocks.data(), n_jobs * sizeof(InflateBlock), hipMemcpyHostToDevice, s));
  if (check) TRY(kInflate, hipMemcpyAsync(base + L.at_crc, want.data(), n_jobs * 4, hipMemcpyHostToDevice, s));
  if (lap.on) {
    TRY(kInflate, launch_bgzf_inflate(ip, s, 1));
    TRY(kInflate, hipStreamSynchronize(s));
    lap("decode kernel");
    TRY(kInflate, launch_bgzf_inflate(ip, s, 2));
    TRY(kInflate, hipStreamSynchronize(s));
    lap("resolve kernel");
  } else {
    TRY(kInflate, launch_bgzf_inflate(ip, s));
  }
  std::vector<uint32_t> status(n_jobs);
  TRY(kInflate, hipMemcpyAsync(status.data(), ip.status, n_jobs * 4, hipMemcpyDeviceToHost, s));
  TRY(kInflate, hipStreamSynchronize(s));
  lap("kernel");
  bool again = false;
  const int32_t ast = inflate_again(kInflate, ip, blocks.data(), check ? want.data() : nullptr, status, s, &again, err256);
  if (ast != MIDAS_SNPS_OK) return ast;
  if (again) lap("streams decoded again");
  for (size_t k = 0; k < n_jobs; ++k) {
    if (status[k] != 0u) {
      if (bad_job) *bad_job = (int64_t)k;
      if (err256) snprintf(err256, 256, status[k] == kInflateCrc ? "CRC-32 mismatch (stream %lld: the inflated bytes are not the ones that were compressed)"
                                                                 : "corrupt deflate data (stream %lld: code %u)", (long long)k, status[k]);
      return MIDAS_SNPS_ERR_BAD_LAYOUT;
    }
  }
  const int32_t st = copy_to_host(ctx, out, base, out_bytes);
  if (st != MIDAS_SNPS_OK && err256) snprintf(err256, 256, "device inflate: results to host: %s", ctx->error_text().c_str());
  lap("inflated bytes down");
  if (st == MIDAS_SNPS_OK && iu->keep) {     // the caller takes the arena: the inflated stream, and everything behind it as scratch
    iu->kept = arena.p; iu->kept_bytes = out_bytes; iu->scratch = base + L.at_comp; iu->scratch_bytes = L.end - L.at_comp;
    arena.p = nullptr;
  }
  return st;
}

// The decode with the host walking the records (the inflated stream comes down for that): what midas_bam_load_device falls back
// to when the device cannot settle the record boundaries.
int32_t bam_load_device_host_walk(const char* path, midas_snps_ctx* ctx, midas_bam** out, int64_t* n_reads, int64_t* seq_bytes,
                                  int64_t* qual_bytes, int64_t* n_cigar, char* err256) {
  if (!ctx || !path || !out) return MIDAS_SNPS_ERR_INVALID_ARG;
  *out = nullptr;
  InflateUser iu{ctx};
  iu.keep = true;
  Lap lap{"device decode", 26};
  struct Kept { InflateUser* u; ~Kept() { if (u->kept) (void)hipFree(u->kept); } } kept{&iu};       // (freed on every way out)
  const BlockInflater inf{&iu, device_inflate};
  midas_bam* b = nullptr;
  int32_t st = bam_open_with(path, &inf, &b, err256);
  if (st != MIDAS_SNPS_OK) return st;
  struct Handle { midas_bam* b; ~Handle() { if (b) midas_bam_close(b); } } handle{b};
  lap("open (map, inflate, header)");
  bam_keep_payload_on_device(b);
  int64_t n = 0, sb = 0, qb = 0, nc = 0;
  st = midas_bam_load(b, &n, &sb, &qb, &nc, err256);        // the host walks the records and decodes the small columns
  if (st != MIDAS_SNPS_OK) return st;
  lap("host walk + small columns");
  size_t n_off = 0;
  const uint64_t* rec_off = bam_record_offsets(b, &n_off);
  const int64_t *seq_off, *qual_off, *cigar_off;
  bam_offsets(b, &seq_off, &qual_off, &cigar_off);
  {
    std::lock_guard<std::mutex> g(ctx->device_mutex);
    TRY(kDecode, hipSetDevice(ctx->device));
    // the columns and the offsets the cut needs go where the compressed bytes and the match lists were (the arena's scratch is
    // 2.7 x the stream, the columns 0.9 x): no second allocation
    struct View { void* p = nullptr; } d_rec, d_so, d_qo, d_co, d_seq, d_qual, d_cig;
    const size_t n1 = (size_t)n + 1;
    size_t at = 0;
    auto take = [&](View& v, size_t bytes) { v.p = iu.scratch + at; at += round256(bytes); };
    take(d_seq, (size_t)sb + 64); take(d_qual, (size_t)qb + 64); take(d_cig, (size_t)nc * 4 + 64);
    take(d_rec, n1 * 8); take(d_so, n1 * 8); take(d_qo, n1 * 8); take(d_co, n1 * 8);
    DeviceBuf own;
    if (at > iu.scratch_bytes) {      // (very short reads: more offsets than the scratch has room for -- a buffer of their own)
      TRY(kDecode, hipMalloc(&own.p, at));
      const ptrdiff_t shift = static_cast<uint8_t*>(own.p) - iu.scratch;
      for (View* v : {&d_seq, &d_qual, &d_cig, &d_rec, &d_so, &d_qo, &d_co}) v->p = static_cast<uint8_t*>(v->p) + shift;
    }
    hipStream_t s = ctx->stream;
    lap("hipMalloc of the columns");
    if (n > 0) TRY(kDecode, hipMemcpyAsync(d_rec.p, rec_off, (size_t)n * 8, hipMemcpyHostToDevice, s));
    TRY(kDecode, hipMemcpyAsync(d_so.p, seq_off, n1 * 8, hipMemcpyHostToDevice, s));
    TRY(kDecode, hipMemcpyAsync(d_qo.p, qual_off, n1 * 8, hipMemcpyHostToDevice, s));
    TRY(kDecode, hipMemcpyAsync(d_co.p, cigar_off, n1 * 8, hipMemcpyHostToDevice, s));
    TRY(kDecode, hipMemsetAsync(static_cast<uint8_t*>(d_cig.p) + (size_t)nc * 4, 0, 64, s));
    if (lap.on) { TRY(kDecode, hipStreamSynchronize(s)); lap("offsets up"); }
    PayloadParams pp;
    pp.stream = static_cast<const uint8_t*>(iu.kept);
    pp.rec_off = static_cast<const unsigned long long*>(d_rec.p);
    pp.n_records = n;
    pp.seq_off = static_cast<const long long*>(d_so.p);
    pp.qual_off = static_cast<const long long*>(d_qo.p);
    pp.cigar_off = static_cast<const long long*>(d_co.p);
    pp.seq4 = static_cast<uint8_t*>(d_seq.p);
    pp.qual = static_cast<uint8_t*>(d_qual.p);
    pp.cigar = static_cast<uint32_t*>(d_cig.p);
    TRY(kDecode, launch_bam_payload(pp, ctx->prop.multiProcessorCount, s));
    TRY(kDecode, hipStreamSynchronize(s));
    lap("payload kernel");
    if (own.p) {                      // (the columns have their own buffer: the arena goes now)
      bam_set_device_payload(b, d_seq.p, d_qual.p, d_cig.p, own.p, device_free);
      own.p = nullptr;
    } else {
      bam_set_device_payload(b, d_seq.p, d_qual.p, d_cig.p, iu.kept, device_free);     // (the arena lives as long as the columns)
      iu.kept = nullptr;
    }
  }
  lap("free scratch");
  if (n_reads) *n_reads = n;
  if (seq_bytes) *seq_bytes = sb;
  if (qual_bytes) *qual_bytes = qb;
  if (n_cigar) *n_cigar = nc;
  *out = b;
  handle.b = nullptr;
  return MIDAS_SNPS_OK;
}

struct ArenaLoan { std::shared_ptr<midas_arena_pool> pool; void* p; };
void arena_loan_free(void* v) {
  ArenaLoan* l = static_cast<ArenaLoan*>(v);
  if (l) { l->pool->drop_twins(l->p); l->pool->give(l->p); delete l; }
}

// ---- the record walk's steps ----------------------------------------------------------------------------------------------------
// The tables of a walk (bam_walk.hip) over the chunks `h` holds: carved out of a scratch region, sent up, walked, the six result
// columns brought down; one chunk walked again from where the chain stands (the callback of decode_plan.h stitch_chunks); and what
// the stitching settled sent up again for the offsets kernel.
struct WalkTables {
  const char* who;        // whose walk: the prefix of its error texts
  char* err256;
  ChunkWalk h;
  BamWalkParams wp;
  long long* d_ref_lens = nullptr;
  unsigned long long *d_lo = nullptr, *d_hi = nullptr, *d_stop = nullptr, *d_limit = nullptr, *d_base = nullptr;
  uint8_t* d_forced = nullptr;
  long long* d_list = nullptr;
  bool carve(Scratch& sc, const uint8_t* stream, int32_t n_ref) {       // false: the region is too small
    const size_t nc1 = std::max<size_t>(h.size(), 1);
    wp.d = stream; wp.n_ref = n_ref; wp.n_chunks = (long long)h.size();
    d_ref_lens = sc.as<long long>((size_t)(n_ref > 0 ? n_ref : 1) * 8);
    d_lo = sc.as<unsigned long long>(nc1 * 8);
    d_hi = sc.as<unsigned long long>(nc1 * 8);
    d_stop = sc.as<unsigned long long>(nc1 * 8);
    d_limit = sc.as<unsigned long long>(nc1 * 8);
    d_forced = sc.take(nc1);
    wp.start = sc.as<unsigned long long>(nc1 * 8);
    wp.end = sc.as<unsigned long long>(nc1 * 8);
    wp.kept = sc.as<uint32_t>(nc1 * 4);
    wp.unmapped = sc.as<uint32_t>(nc1 * 4);
    wp.first_unmapped = sc.as<unsigned long long>(nc1 * 8);
    wp.bad = sc.as<uint32_t>(nc1 * 4);
    d_base = sc.as<unsigned long long>(nc1 * 8);
    d_list = sc.as<long long>(4096 * 8);
    wp.lo = d_lo; wp.hi = d_hi; wp.stop = d_stop; wp.limit = d_limit; wp.forced = d_forced; wp.ref_lens = d_ref_lens;
    h.room_for_results();
    return d_list != nullptr;
  }
  int32_t walk(const int64_t* ref_lens, hipStream_t s) {
    const size_t n = h.size();
    if (wp.n_ref > 0) TRY(who, hipMemcpyAsync(d_ref_lens, ref_lens, (size_t)wp.n_ref * 8, hipMemcpyHostToDevice, s));
    if (n == 0) return MIDAS_SNPS_OK;
    TRY(who, hipMemcpyAsync(d_lo, h.lo.data(), n * 8, hipMemcpyHostToDevice, s));
    TRY(who, hipMemcpyAsync(d_hi, h.hi.data(), n * 8, hipMemcpyHostToDevice, s));
    TRY(who, hipMemcpyAsync(d_stop, h.stop.data(), n * 8, hipMemcpyHostToDevice, s));
    TRY(who, hipMemcpyAsync(d_limit, h.limit.data(), n * 8, hipMemcpyHostToDevice, s));
    TRY(who, hipMemcpyAsync(d_forced, h.forced.data(), n, hipMemcpyHostToDevice, s));
    TRY(who, hipMemcpyAsync(wp.start, h.start.data(), n * 8, hipMemcpyHostToDevice, s));
    TRY(who, launch_bam_walk(wp, nullptr, 0, s));
    TRY(who, hipMemcpyAsync(h.start.data(), wp.start, n * 8, hipMemcpyDeviceToHost, s));
    TRY(who, hipMemcpyAsync(h.end.data(), wp.end, n * 8, hipMemcpyDeviceToHost, s));
    TRY(who, hipMemcpyAsync(h.kept.data(), wp.kept, n * 4, hipMemcpyDeviceToHost, s));
    TRY(who, hipMemcpyAsync(h.unmapped.data(), wp.unmapped, n * 4, hipMemcpyDeviceToHost, s));
    TRY(who, hipMemcpyAsync(h.first_unmapped.data(), wp.first_unmapped, n * 8, hipMemcpyDeviceToHost, s));
    TRY(who, hipMemcpyAsync(h.bad.data(), wp.bad, n * 4, hipMemcpyDeviceToHost, s));
    TRY(who, hipStreamSynchronize(s));
    return MIDAS_SNPS_OK;
  }
  int32_t walk_again(size_t c, unsigned long long cur, hipStream_t s) {
    const long long one = (long long)c;
    TRY(who, hipMemcpyAsync(wp.start + c, &cur, 8, hipMemcpyHostToDevice, s));
    TRY(who, hipMemcpyAsync(d_list, &one, 8, hipMemcpyHostToDevice, s));
    TRY(who, launch_bam_walk(wp, d_list, 1, s));
    TRY(who, hipMemcpyAsync(&h.end[c], wp.end + c, 8, hipMemcpyDeviceToHost, s));
    TRY(who, hipMemcpyAsync(&h.kept[c], wp.kept + c, 4, hipMemcpyDeviceToHost, s));
    TRY(who, hipMemcpyAsync(&h.unmapped[c], wp.unmapped + c, 4, hipMemcpyDeviceToHost, s));
    TRY(who, hipMemcpyAsync(&h.first_unmapped[c], wp.first_unmapped + c, 8, hipMemcpyDeviceToHost, s));
    TRY(who, hipMemcpyAsync(&h.bad[c], wp.bad + c, 4, hipMemcpyDeviceToHost, s));
    TRY(who, hipStreamSynchronize(s));
    h.start[c] = cur;
    return MIDAS_SNPS_OK;
  }
  int32_t settled_up(hipStream_t s) {        // (after ChunkWalk::count_records)
    const size_t n = h.size();
    if (n == 0) return MIDAS_SNPS_OK;
    TRY(who, hipMemcpyAsync(wp.start, h.start.data(), n * 8, hipMemcpyHostToDevice, s));
    TRY(who, hipMemcpyAsync(wp.kept, h.kept.data(), n * 4, hipMemcpyHostToDevice, s));
    TRY(who, hipMemcpyAsync(d_base, h.base.data(), n * 8, hipMemcpyHostToDevice, s));
    return MIDAS_SNPS_OK;
  }
};

// Every record's offset (the chunks' settled starts and counts) and its columns: cp.bad_record cleared, the two kernels, then
// *bad_record and where the offset columns ended come down, waited for.
int32_t run_columns(const WalkTables& walk, unsigned long long* d_rec, const BamColumnsParams& cp, long long* d_scan, hipStream_t s,
                    unsigned long long* bad_record, long long ends[4]) {
  const char* const who = walk.who;
  char* const err256 = walk.err256;
  TRY(who, hipMemsetAsync(cp.bad_record, 0xFF, 8, s));
  TRY(who, launch_bam_offsets(walk.wp, walk.d_base, d_rec, s));
  TRY(who, launch_bam_columns(cp, d_scan, s));
  TRY(who, hipMemcpyAsync(bad_record, cp.bad_record, 8, hipMemcpyDeviceToHost, s));
  long long* const last[4] = {cp.seq_off, cp.qual_off, cp.cigar_off, cp.unit_off};
  for (int k = 0; k < 4; ++k)
    if (last[k]) TRY(who, hipMemcpyAsync(&ends[k], last[k] + cp.n, 8, hipMemcpyDeviceToHost, s));
  TRY(who, hipStreamSynchronize(s));
  return MIDAS_SNPS_OK;
}

// ---- the streamed decode ------------------------------------------------------------------------------------------------------
// A BAM of several device-fills of blocks (bgzf_inflate_wave_blocks), decoded RESIDENT group by group: the reference's loop over the
// file (midas/run/snps.py:186-199 iterates the alignments as htslib inflates them, a block at a time) at the device's granularity.
//   * a GROUP is a run of whole BGZF blocks -- one wave of the decoder's workgroups by default -- plus a few blocks behind it for
//     the record that straddles its end; it wants the records that START inside it.  Where the chain of group g ends (the first
//     record start at or behind its last wanted byte) is the exact first record of group g + 1: nothing is guessed behind group 0.
//   * a group lives in a SLOT (inflated bytes | compressed bytes | block tables | match lists, the walk's tables over the dead
//     ones); an uploader thread fills slot (g + 1) % S through the pinned ring on a stream of its own while the kernels of group g
//     run on the context's -- the link and the decoder work at the same time.
//   * what STAYS is written where it stays: every group's columns continue the ones before it (BamColumnsParams::base: the offset
//     scans start at what the earlier groups came to), its records and their [cigar][seq][qual] runs go straight behind theirs
//     in the direct layout.  Those arrays are sized from the first group's records per inflated byte (+ 3 %) and grown (a copy on
//     the device) if a later group proves the estimate short.
// Device memory: S slots of ~2.5 x a group's inflated bytes + the result (~1.1 x the file's inflated bytes), against ~2.3 x the
// file's inflated bytes in one arena -- bounded by the group, not by the file, in everything but the result itself.
// No inflated stream is kept: a handle decoded this way cuts its raw columns, if somebody asks for them, out of the direct layout
// (PayloadParams::drec).  kStreamFallback: this BAM is not for the streamed decode (a record longer than the blocks a group
// keeps behind its end) -- the caller decodes it in one arena.
constexpr int32_t kStreamFallback = -1000;
constexpr size_t kTail = 8;                                  // blocks kept behind a group's last: the record that straddles its end lies in them
constexpr uint32_t kSideFirstEntries = 4096;                 // the side buffer's first room (layout.h DenseSide): grown by the group that needs more
constexpr unsigned long long kSideFirstBytes = 1ull << 20;

// The uploader: a group's bytes and tables up on its own stream, then the group's decoder / resolver / CRC kernels on one of two
// streams (groups alternate: the decoder is latency-bound -- ~25 ms a launch however few blocks -- and the next group's workgroups
// fill the CUs that this group's stragglers leave idle), its statuses down into pinned memory, an event behind them.  It runs at
// most n_slots groups ahead of the decode.
struct StreamPipe {
  midas_snps_ctx* ctx;
  const uint8_t* comp_base;
  const InflateJob* jobs;
  const StreamPlan& plan;
  uint8_t* arena;
  int n_slots;
  std::mutex m;
  std::condition_variable cv;
  long long launched = 0, decoded = 0;
  bool abort = false;
  int32_t status = MIDAS_SNPS_OK;
  hipError_t hip = hipSuccess;
  double busy_ms = 0;
  struct GroupHost { std::vector<InflateBlock> blocks; std::vector<uint32_t> want; };
  std::vector<GroupHost> host;
  hipStream_t up = nullptr, inf[2] = {nullptr, nullptr};
  std::vector<hipEvent_t> ev;
  uint32_t* status_down = nullptr;      // pinned: every group's block statuses, group g's from status_at[g] on
  std::vector<size_t> status_at;
  std::thread uploader;

  uint8_t* slot(size_t g) const { return arena + (g % (size_t)n_slots) * plan.slot_bytes; }
  int32_t start(char* err256) {
    const size_t K = plan.groups.size();
    host.resize(K);
    TRY(kStreamed, hipStreamCreateWithFlags(&up, hipStreamNonBlocking));
    TRY(kStreamed, hipStreamCreateWithFlags(&inf[0], hipStreamNonBlocking));
    TRY(kStreamed, hipStreamCreateWithFlags(&inf[1], hipStreamNonBlocking));
    ev.assign(K, nullptr);
    for (size_t g = 0; g < K; ++g) TRY(kStreamed, hipEventCreateWithFlags(&ev[g], hipEventDisableTiming));
    status_at.assign(K + 1, 0);
    for (size_t g = 0; g < K; ++g) status_at[g + 1] = status_at[g] + plan.groups[g].n_blocks();
    TRY(kStreamed, hipHostMalloc(reinterpret_cast<void**>(&status_down), status_at[K] * 4 + 64, kHostAllocFlags));
    uploader = std::thread([this] { upload_groups(); });
    return MIDAS_SNPS_OK;
  }
  void upload_groups() {
    (void)hipSetDevice(ctx->device);
    for (size_t g = 0; g < plan.groups.size(); ++g) {
      {
        std::unique_lock<std::mutex> lk(m);
        cv.wait(lk, [&] { return abort || (long long)g < decoded + n_slots; });
        if (abort) return;
      }
      const DecodeGroup& G = plan.groups[g];
      uint8_t* const to = slot(g);
      const auto t0 = Clock::now();
      const size_t nj = G.n_blocks();
      GroupHost& H = host[g];
      H.blocks.resize(nj);
      H.want.resize(nj);
      unsigned long long room = 0;
      fill_inflate_blocks(jobs + G.b_lo, nj, jobs[G.b_lo].cpos, 0, G.u_lo, H.blocks.data(), H.want.data(), &room);
      const InflateLayout L = G.layout();
      int32_t ust = copy_to_device_staged(ctx, to + L.at_comp, comp_base + jobs[G.b_lo].cpos, G.comp, up);
      hipError_t e = hipSuccess;
      if (ust == MIDAS_SNPS_OK) {
        e = hipMemcpyAsync(to + L.at_blocks, H.blocks.data(), nj * sizeof(InflateBlock), hipMemcpyHostToDevice, up);
        if (e == hipSuccess) e = hipMemcpyAsync(to + L.at_crc, H.want.data(), nj * 4, hipMemcpyHostToDevice, up);
        if (e == hipSuccess) e = hipMemsetAsync(to + L.at_comp + G.comp, 0, 512, up);
        if (e == hipSuccess) e = hipStreamSynchronize(up);
        if (e == hipSuccess) {
          hipStream_t q = inf[g & 1];
          const InflateParams ip = inflate_params(L, to, nj);
          e = launch_bgzf_inflate(ip, q);
          if (e == hipSuccess) e = hipMemcpyAsync(status_down + status_at[g], ip.status, nj * 4, hipMemcpyDeviceToHost, q);
          if (e == hipSuccess) e = hipEventRecord(ev[g], q);
        }
        if (e != hipSuccess) { (void)hipGetLastError(); ust = e == hipErrorOutOfMemory ? MIDAS_SNPS_ERR_OUT_OF_MEMORY : MIDAS_SNPS_ERR_HIP; }
      }
      {
        std::lock_guard<std::mutex> lk(m);
        busy_ms += ms_since(t0);
        if (ust != MIDAS_SNPS_OK) { status = ust; hip = e; abort = true; }
        else launched = (long long)g + 1;
      }
      cv.notify_all();
      if (ust != MIDAS_SNPS_OK) return;
    }
  }
  // until group g's kernels are launched (its event says when they are done)
  int32_t wait_launched(size_t g, char* err256) {
    std::unique_lock<std::mutex> lk(m);
    cv.wait(lk, [&] { return abort || launched > (long long)g; });
    if (launched > (long long)g) return MIDAS_SNPS_OK;
    if (hip != hipSuccess) return hip_err(err256, kStreamed, hip, "a group's blocks to the device and its decoder's launch");
    if (err256) snprintf(err256, 256, "device decode (streamed): blocks to the device: %s", ctx->error_text().c_str());
    return status != MIDAS_SNPS_OK ? status : MIDAS_SNPS_ERR_HIP;
  }
  void group_decoded(size_t g) {        // its slot is the uploader's again
    { std::lock_guard<std::mutex> lk(m); decoded = (long long)g + 1; }
    cv.notify_all();
  }
  void stop() {       // the uploader is told to stop and waited for
    { std::lock_guard<std::mutex> lk(m); abort = true; }
    cv.notify_all();
    if (uploader.joinable()) uploader.join();
  }
  ~StreamPipe() {     // (every way out: the uploader first, then the streams' work, then the streams)
    stop();
    for (hipStream_t q : inf) if (q) (void)hipStreamSynchronize(q);
    (void)hipGetLastError();
    for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
    if (up) (void)hipStreamDestroy(up);
    for (hipStream_t q : inf) if (q) (void)hipStreamDestroy(q);
    if (status_down) (void)hipHostFree(status_down);
  }
};

// The result of a streamed decode: the records' arrays, the direct layout's payload and the side buffer, each its own allocation,
// grown (what the groups so far wrote moves along) when a group needs more; the handle takes the three when the decode is done.
struct TwoBuffers { void* a; void* b; void* c; };
void two_buffers_free(void* v) {
  TwoBuffers* t = static_cast<TwoBuffers*>(v);
  if (t->a) (void)hipFree(t->a);
  if (t->b) (void)hipFree(t->b);
  if (t->c) (void)hipFree(t->c);
  delete t;
}
struct StreamColumns {       // the result's record arrays in ONE allocation, for `cap` records (+ 2: the offsets' last entry, the sentinel record)
  uint8_t* p = nullptr;
  size_t cap = 0, bytes = 0;
  size_t at[11] = {0};        // rec, refid, pos, nm, l_seq, mapq, flag, seq_off, qual_off, cigar_off, unit_off
  static constexpr size_t width(int k) { return k == 0 ? 16 : (k <= 4 ? 4 : (k == 5 ? 1 : (k == 6 ? 2 : 8))); }
  void lay(size_t cap_records) {
    cap = cap_records;
    size_t o = 0;
    for (int k = 0; k < 11; ++k) { at[k] = o; o += round256((cap + 2) * width(k)); }
    bytes = o;
  }
  template <class T> T* col(int k) const { return reinterpret_cast<T*>(p + at[k]); }
};
struct StreamResult {
  hipStream_t s;
  char* err256;
  StreamColumns cols;
  uint8_t* pay = nullptr;
  size_t pay_cap_units = 0;
  // the side buffer (layout.h DenseSide): the raw SEQ / QUAL of the reads the base bytes cannot give back -- none in most files;
  // a group that finds no room is written again behind a buffer with room for all of its SEQ / QUAL
  DenseSide* side = nullptr;
  DenseSide side_h{};
  long long N = 0;                                  // records so far
  long long base[4] = {0, 0, 0, 0};                 // what the offset columns came to so far: SEQ bytes, QUAL bytes, CIGAR ops, payload units
  int regrown = 0;
  bool handed_over = false;
  ~StreamResult() {
    if (handed_over) return;
    if (cols.p) (void)hipFree(cols.p);
    if (pay) (void)hipFree(pay);
    if (side) (void)hipFree(side);
  }
  unsigned long long side_entries() const { return side_h.bump >> kDenseSideEntryShift; }
  unsigned long long side_bytes() const { return (side_h.bump & kDenseSideMaxField) << 3; }
  int32_t grow_side(uint32_t cap_entries, unsigned long long cap_bytes) {
    DenseSide* q = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&q), (size_t)dense_side_bytes(cap_entries, cap_bytes));
    if (e != hipSuccess) return hip_err(err256, kStreamed, e, "the side buffer");
    DenseSide h = side_h;
    h.flags &= ~kDenseSideOverflow;
    h.cap_entries = cap_entries; h.cap_bytes = cap_bytes;
    e = hipMemcpyAsync(q, &h, sizeof h, hipMemcpyHostToDevice, s);
    if (side && side_entries() > 0) {
      if (e == hipSuccess) e = hipMemcpyAsync(dense_side_entries(q), dense_side_entries(side), side_entries() * sizeof(DenseSideEntry), hipMemcpyDeviceToDevice, s);
      if (e == hipSuccess) e = hipMemcpyAsync(reinterpret_cast<uint8_t*>(dense_side_entries(q) + cap_entries),
                                              reinterpret_cast<uint8_t*>(dense_side_entries(side) + side_h.cap_entries), side_bytes(), hipMemcpyDeviceToDevice, s);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (side) (void)hipFree(side);
    side = q;
    side_h = h;
    return e == hipSuccess ? MIDAS_SNPS_OK : hip_err(err256, kStreamed, e, "the side buffer moved");
  }
  int32_t grow_columns(size_t need) {       // room for `need` records
    if (cols.p && need <= cols.cap) return MIDAS_SNPS_OK;
    StreamColumns nc;
    nc.lay(need);
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&nc.p), nc.bytes);
    if (e != hipSuccess) return hip_err(err256, kStreamed, e, "the records' arrays");
    if (cols.p) {
      for (int k = 0; k < 11; ++k) {
        const size_t n = (size_t)N + (k == 0 || k >= 7 ? 1 : 0);
        e = hipMemcpyAsync(nc.p + nc.at[k], cols.p + cols.at[k], n * StreamColumns::width(k), hipMemcpyDeviceToDevice, s);
        if (e != hipSuccess) { (void)hipFree(nc.p); return hip_err(err256, kStreamed, e, "the records' arrays moved"); }
      }
      e = hipStreamSynchronize(s);
      (void)hipFree(cols.p);
      if (e != hipSuccess) { (void)hipFree(nc.p); return hip_err(err256, kStreamed, e, "the records' arrays moved"); }
    }
    cols = nc;
    return MIDAS_SNPS_OK;
  }
  int32_t grow_payload(size_t need_units) {
    if (pay && need_units <= pay_cap_units) return MIDAS_SNPS_OK;
    uint8_t* q = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&q), need_units * 8 + 64);
    if (e != hipSuccess) return hip_err(err256, kStreamed, e, "the reads' payload");
    if (pay) {
      e = base[3] > 0 ? hipMemcpyAsync(q, pay, (size_t)base[3] * 8, hipMemcpyDeviceToDevice, s) : hipSuccess;
      if (e == hipSuccess) e = hipStreamSynchronize(s);
      (void)hipFree(pay);
      if (e != hipSuccess) { (void)hipFree(q); return hip_err(err256, kStreamed, e, "the reads' payload moved"); }
    }
    pay = q;
    pay_cap_units = need_units;
    return MIDAS_SNPS_OK;
  }
  void hand_over(DeviceDecodeResult* res) {
    res->n_records = N; res->seq_bytes = base[0]; res->qual_bytes = base[1]; res->n_cigar = base[2];
    ResidentReads& rr = res->resident;
    rr.rec = cols.col<DirectRec>(0); rr.payload = pay; rr.refid = cols.col<int32_t>(1); rr.pos = cols.col<int32_t>(2); rr.nm = cols.col<int32_t>(3);
    rr.l_seq = cols.col<int32_t>(4); rr.mapq = cols.col<uint8_t>(5); rr.flag = cols.col<uint16_t>(6);
    rr.seq_off = cols.col<int64_t>(7); rr.qual_off = cols.col<int64_t>(8); rr.cigar_off = cols.col<int64_t>(9); rr.unit_off = cols.col<int64_t>(10);
    rr.stream = nullptr; rr.rec_off = nullptr;       // (no inflated stream is kept: raw columns come out of the direct layout)
    rr.payload_units = base[3];
    rr.side = side;
    rr.dense_flags = side_h.flags;
    res->dev_owner = new TwoBuffers{cols.p, pay, side};
    res->dev_free = two_buffers_free;
    handed_over = true;
  }
};

// One streamed decode: what its groups share, and the two steps of a group.
struct StreamDecode {
  midas_snps_ctx* ctx;
  DecodeSegment& sg;
  const StreamPlan& plan;
  StreamPipe& pipe;
  StreamResult& out;
  const int64_t* ref_lens;
  int32_t n_ref;
  int64_t* bad_job;
  int64_t* bad_record;
  char* err256;
  unsigned long long cur;        // GLOBAL buffer offset of the next record (none: group 0 guesses it)
  double span_total;
  Lap lap{"device decode", 0};
  double laps[8] = {0, 0, 0, 0, 0, 0, 0, 0};     // waited for the upload, inflate, walk, stitch, columns, direct, grow, tables
  int rounds = 0;

  // the wanted bytes over the bytes walked so far: the result's arrays are sized from the records per inflated byte so far (+ 3 %)
  double share() const { return std::max(1.0, span_total / (double)(cur != kNoOffset && cur > sg.from ? cur - sg.from : 1)); }

  // status wait -> second pass -> walk -> stitch, then write_group for what the group holds
  int32_t decode_group(size_t g) {
    const DecodeGroup& G = plan.groups[g];
    uint8_t* const slot = pipe.slot(g);
    const InflateLayout L = G.layout();
    hipStream_t s = ctx->stream;
    laps[7] += lap.take();
    const int32_t wst = pipe.wait_launched(g, err256);
    if (wst != MIDAS_SNPS_OK) return wst;
    laps[0] += lap.take();
    TRY(kStreamed, hipEventSynchronize(pipe.ev[g]));        // the group is inflated, resolved, checked; its statuses are down
    std::vector<uint32_t> status(pipe.status_down + pipe.status_at[g], pipe.status_down + pipe.status_at[g + 1]);
    bool again = false;
    const int32_t ast = inflate_again(kStreamed, inflate_params(L, slot, G.n_blocks()), pipe.host[g].blocks.data(), pipe.host[g].want.data(), status, s, &again, err256);
    if (ast != MIDAS_SNPS_OK) return ast;
    if (check_block_statuses(status, G.b_lo, bad_job, err256) != MIDAS_SNPS_OK) return MIDAS_SNPS_ERR_BAD_LAYOUT;
    laps[1] += lap.take();
    // ---- the record walk of the group: chunks over [from, stop) in the slot's own offsets -----------------------------------------
    if (cur != kNoOffset && cur < G.u_lo) {        // (cannot be: the chain of the group before ended at or behind this group's first byte)
      if (err256) snprintf(err256, 256, "device decode (streamed): the record chain fell behind group %zu", g);
      return MIDAS_SNPS_ERR_UNSUPPORTED;
    }
    const bool exact = cur != kNoOffset;
    const unsigned long long l_from = exact ? cur - G.u_lo : (g == 0 && sg.from >= G.u_lo ? (unsigned long long)(sg.from - G.u_lo) : 0ull);
    const unsigned long long l_stop = G.stop > G.u_lo ? (unsigned long long)(G.stop - G.u_lo) : 0ull;
    WalkTables walk{kStreamed, err256};
    walk.h.add_segment(l_from, l_stop, G.infl, exact);
    Scratch sc{slot + L.at_comp, plan.slot_bytes - L.at_comp};
    if (!walk.carve(sc, slot, n_ref)) { if (err256) snprintf(err256, 256, "device decode (streamed): a slot is too small for the walk"); return MIDAS_SNPS_ERR_OUT_OF_MEMORY; }
    const int32_t walked = walk.walk(ref_lens, s);
    if (walked != MIDAS_SNPS_OK) return walked;
    laps[2] += lap.take();
    // a record that overruns the bytes the group keeps behind its end: not for this decode
    int32_t again_st = MIDAS_SNPS_OK;
    const StitchResult r = stitch_chunks(walk.h, 0, walk.h.size(), exact ? l_from : kNoOffset, &rounds,
                                         [&](size_t c, unsigned long long at) { again_st = walk.walk_again(c, at, s); return again_st == MIDAS_SNPS_OK; });
    if (r.what == Stitch::bad_chunk) {
      if (G.b_ext < sg.job_hi) return kStreamFallback;       // (the group's own bytes end where the record goes on: the one-arena decode holds it whole)
      *bad_record = -2;
      return MIDAS_SNPS_ERR_BAD_LAYOUT;
    }
    if (r.what == Stitch::unsettled) { if (err256) snprintf(err256, 256, "device decode: the record boundaries did not settle"); return MIDAS_SNPS_ERR_UNSUPPORTED; }
    if (r.what == Stitch::failed) return again_st;
    if (r.first_unmapped != kNoOffset && sg.first_unmapped == kNoOffset) sg.first_unmapped = r.first_unmapped + G.u_lo;
    sg.n_unmapped += r.n_unmapped;
    if (r.end != kNoOffset) {      // (else: a group that had to guess found no record boundary: the next one guesses too)
      cur = r.end + G.u_lo;
      sg.end = cur;
    }
    if (r.first != kNoOffset && sg.first == kNoOffset) sg.first = r.first + G.u_lo;
    const long long n = (long long)walk.h.count_records();
    laps[3] += lap.take();
    if (n > 0) {
      const int32_t st = write_group(g, slot, walk, sc, n);
      if (st != MIDAS_SNPS_OK) return st;
    }
    pipe.group_decoded(g);
    return MIDAS_SNPS_OK;
  }

  // columns -> direct layout (with the side buffer's retry): the group's n records behind those of the groups before it
  int32_t write_group(size_t g, uint8_t* slot, WalkTables& walk, Scratch& sc, long long n) {
    hipStream_t s = ctx->stream;
    const long long N = out.N;
    const int32_t up_st = walk.settled_up(s);
    if (up_st != MIDAS_SNPS_OK) return up_st;
    if (!out.cols.p || (size_t)(N + n) > out.cols.cap) {
      if (out.cols.p) ++out.regrown;
      const int32_t gst = out.grow_columns(std::max((size_t)(N + n), (size_t)((double)(N + n) * share() * 1.03 + 4096.0)));
      if (gst != MIDAS_SNPS_OK) return gst;
      laps[6] += lap.take();
    }
    unsigned long long* d_rec = sc.as<unsigned long long>(((size_t)n + 1) * 8);
    unsigned long long* d_badrec = sc.as<unsigned long long>(8);
    long long* d_scan = sc.as<long long>(bam_scan_scratch_bytes(n));
    if (!d_scan) { if (err256) snprintf(err256, 256, "device decode (streamed): a slot is too small for the record offsets"); return MIDAS_SNPS_ERR_OUT_OF_MEMORY; }
    const StreamColumns& cols = out.cols;
    BamColumnsParams cp;
    cp.d = slot; cp.rec_off = d_rec; cp.n = n; cp.n_ref = n_ref;
    cp.refid = cols.col<int32_t>(1) + N; cp.pos = cols.col<int32_t>(2) + N; cp.nm = cols.col<int32_t>(3) + N; cp.l_seq = cols.col<int32_t>(4) + N;
    cp.mapq = cols.col<uint8_t>(5) + N; cp.flag = cols.col<uint16_t>(6) + N;
    cp.seq_off = cols.col<long long>(7) + N; cp.qual_off = cols.col<long long>(8) + N; cp.cigar_off = cols.col<long long>(9) + N;
    cp.unit_off = cols.col<long long>(10) + N;
    cp.span = nullptr;
    cp.bad_record = d_badrec;
    for (int k = 0; k < 4; ++k) cp.base[k] = out.base[k];
    unsigned long long h_bad_record = kNoOffset;
    long long ends[4] = {0, 0, 0, 0};
    const int32_t cst = run_columns(walk, d_rec, cp, d_scan, s, &h_bad_record, ends);
    if (cst != MIDAS_SNPS_OK) return cst;
    laps[4] += lap.take();
    if (h_bad_record != kNoOffset) { *bad_record = (int64_t)h_bad_record + N; return MIDAS_SNPS_ERR_BAD_LAYOUT; }
    if ((unsigned long long)ends[3] > kMaxDirectPayloadUnits) {
      if (err256) snprintf(err256, 256, "device decode: %llu bytes of read payload exceed the 32 GiB the direct layout addresses", (unsigned long long)ends[3] * 8ull);
      return MIDAS_SNPS_ERR_UNSUPPORTED;
    }
    if (!out.pay || (size_t)ends[3] > out.pay_cap_units) {
      const double est = (double)ends[3] * share() * 1.03 + 65536.0;
      if (out.pay) ++out.regrown;
      const int32_t gst = out.grow_payload(std::max((size_t)ends[3], (size_t)std::min(est, (double)kMaxDirectPayloadUnits)));
      if (gst != MIDAS_SNPS_OK) return gst;
      laps[6] += lap.take();
    }
    BamDirectParams dp;
    dp.stream = slot; dp.rec_off = d_rec; dp.n_records = n;
    dp.pos = cp.pos; dp.nm = cp.nm; dp.unit_off = cp.unit_off;
    dp.rec = cols.col<DirectRec>(0) + N; dp.payload = out.pay;
    dp.read_base = N; dp.side_copy = 1;
    // the most this group can reserve: every read an entry, its SEQ + QUAL (8-byte aligned) in data
    const unsigned long long g_ent = (unsigned long long)n, g_bytes = (unsigned long long)(ends[0] - out.base[0]) + (unsigned long long)(ends[1] - out.base[1]) + 8ull * (unsigned long long)n;
    for (int attempt = 0;; ++attempt) {
      const unsigned long long n_ent = out.side_entries(), n_bytes = out.side_bytes();
      if (!dense_side_fits(n_ent + g_ent, (n_bytes + g_bytes) >> 3)) {       // (the bump's fields could carry: refuse, never lose a read)
        if (err256) snprintf(err256, 256, "device decode (streamed): the exact copies of the reads the layout cannot hold exceed the side buffer's limits (%llu reads, %llu bytes)",
                             n_ent + g_ent, n_bytes + g_bytes);
        return MIDAS_SNPS_ERR_UNSUPPORTED;
      }
      dp.side = out.side;
      TRY(kStreamed, launch_bam_direct(dp, ctx->prop.multiProcessorCount, s));
      DenseSide h{};
      TRY(kStreamed, hipMemcpyAsync(&h, out.side, sizeof h, hipMemcpyDeviceToHost, s));
      TRY(kStreamed, hipStreamSynchronize(s));
      if (!(h.flags & kDenseSideOverflow)) { out.side_h = h; break; }
      // no room for the group's exceptional reads: at least room for ALL of its reads' SEQ / QUAL behind what the groups before
      // kept (twice the old room when that is more: a file of exceptional reads grows it a few times, not every group), and the
      // group written again (the bump and the flags as they were in front of it)
      if (attempt > 0) {
        if (err256) snprintf(err256, 256, "device decode (streamed): group %zu found no room in a side buffer sized for all of its reads", g);
        return MIDAS_SNPS_ERR_HIP;
      }
      const unsigned long long want_e = std::min(kDenseSideMaxField, std::max(n_ent + g_ent, 2ull * out.side_h.cap_entries));
      const unsigned long long want_b = std::min(kDenseSideMaxField << 3, std::max(n_bytes + g_bytes, 2ull * out.side_h.cap_bytes));
      const int32_t gs = out.grow_side((uint32_t)want_e, want_b);
      if (gs != MIDAS_SNPS_OK) return gs;
      if (lap.on) fprintf(stderr, "[device decode] streamed: group %zu: the side buffer grown to %llu reads, %llu bytes\n", g, want_e, want_b);
    }
    laps[5] += lap.take();
    out.N += n;
    for (int k = 0; k < 4; ++k) out.base[k] = ends[k];
    return MIDAS_SNPS_OK;
  }
};

int32_t device_decode_stream(midas_snps_ctx* ctx, const uint8_t* comp_base, const InflateJob* jobs, DecodeSegment& sg, size_t group_blocks, int n_slots,
                             const int64_t* ref_lens, int32_t n_ref, HostColumns (*alloc)(void*, int64_t), void* sink, DeviceDecodeResult* res,
                             int64_t* bad_job, int64_t* bad_record, char* err256) {
  const auto t_begin = Clock::now();
  hipStream_t s = ctx->stream;
  const StreamPlan plan = plan_groups(jobs, sg.job_lo, sg.job_hi, group_blocks, kTail, n_ref, sg.stop);
  if (plan.bad_block >= 0) { if (err256) snprintf(err256, 256, "device decode: block %lld lies outside the buffers", (long long)plan.bad_block); return MIDAS_SNPS_ERR_INVALID_ARG; }
  const size_t K = plan.groups.size();
  if (n_slots > (int)K) n_slots = (int)K;
  bool pooled = false;
  void* arena_p = ctx->arena->take(plan.slot_bytes * (size_t)n_slots, &pooled);
  if (!arena_p) { if (err256) snprintf(err256, 256, "device decode (streamed): out of device memory (%.1f GB of slots)", (double)(plan.slot_bytes * (size_t)n_slots) / 1e9); return MIDAS_SNPS_ERR_OUT_OF_MEMORY; }
  Loan loan{ctx->arena, arena_p};
  const bool trace = getenv("MIDAS_SNPS_TRACE") != nullptr;
  if (trace) fprintf(stderr, "[device decode] streamed: %zu groups of <= %zu blocks, %d slots of %.2f GB (allocated in %.1f ms)\n", K, group_blocks, n_slots,
                     (double)plan.slot_bytes / 1e9, ms_since(t_begin));
  // (in this order: on every way out the result goes first, then the uploader is stopped and waited for, then the slots go back)
  StreamPipe pipe{ctx, comp_base, jobs, plan, static_cast<uint8_t*>(arena_p), n_slots};
  StreamResult out{s, err256};
  sg.first = kNoOffset; sg.n_records = 0; sg.n_unmapped = 0; sg.first_unmapped = kNoOffset; sg.end = plan.seg_stop;
  StreamDecode dec{ctx, sg, plan, pipe, out, ref_lens, n_ref, bad_job, bad_record, err256, sg.exact ? sg.from : kNoOffset,
                   (double)(plan.seg_stop > sg.from ? plan.seg_stop - sg.from : 1)};
  const int32_t pst = pipe.start(err256);
  if (pst != MIDAS_SNPS_OK) return pst;
  const int32_t gs = out.grow_side(kSideFirstEntries, kSideFirstBytes);
  if (gs != MIDAS_SNPS_OK) return gs;
  for (size_t g = 0; g < K; ++g) {
    const int32_t st = dec.decode_group(g);
    if (st != MIDAS_SNPS_OK) return st;
    if (dec.cur != kNoOffset && dec.cur >= plan.seg_stop) break;       // (the wanted records end here: nothing of the groups behind is needed)
  }
  const long long N = out.N;
  sg.n_records = N;
  if (N == 0) {        // (no record at all: the caller's columns are empty; nothing stays on the device)
    (void)alloc(sink, 0);
    const int32_t g0 = out.grow_columns(1);
    if (g0 != MIDAS_SNPS_OK) return g0;
    const int32_t g1 = out.grow_payload(8);
    if (g1 != MIDAS_SNPS_OK) return g1;
    TRY(kStreamed, hipMemsetAsync(out.cols.p, 0, out.cols.bytes, s));
  }
  TRY(kStreamed, hipMemsetAsync(out.pay + (size_t)out.base[3] * 8, 0, 64, s));      // (a lane's 16-byte loads may overhang the last read)
  pipe.stop();        // the uploader has nothing left to do: the ring is the copy-down's again
  for (hipStream_t q : pipe.inf) TRY(kStreamed, hipStreamSynchronize(q));
  if (N > 0) {
    const HostColumns hc = alloc(sink, N);
    if (!hc.refid) { TRY(kStreamed, hipStreamSynchronize(s)); return MIDAS_SNPS_OK; }
    const int32_t dst = copy_to_host(ctx, hc.refid, out.cols.col<int32_t>(1), (size_t)N * 4);
    if (dst != MIDAS_SNPS_OK) { if (err256) snprintf(err256, 256, "device decode: columns to host: %s", ctx->error_text().c_str()); return dst; }
  }
  TRY(kStreamed, hipStreamSynchronize(s));
  if (trace) {
    const double* laps = dec.laps;
    fprintf(stderr, "[device decode] streamed: %lld records in %.1f ms: waited for a group's launch %.1f (the uploader worked %.1f), for its decoder %.1f, walk %.1f, stitch %.1f, "
                    "columns %.1f, direct layout %.1f, result grown %.1f (%d times), tables %.1f ms; %d chunk(s) walked again; result %.2f GB\n",
            N, ms_since(t_begin), laps[0], pipe.busy_ms, laps[1], laps[2], laps[3], laps[4], laps[5], laps[6], out.regrown, laps[7], dec.rounds,
            (double)(out.cols.bytes + out.pay_cap_units * 8) / 1e9);
  }
  out.hand_over(res);
  return MIDAS_SNPS_OK;
}

// A resident decode of ONE run of blocks that fills the device several times over goes group by group (device_decode_stream).
// kStreamFallback: it is not such a decode, or the streamed decode gave up on it -- one arena.
int32_t decode_streamed_if_large(midas_snps_ctx* ctx, const uint8_t* comp_base, const InflateJob* jobs, size_t n_jobs, DecodeSegment* segs, size_t n_segs,
                                 const int64_t* ref_lens, int32_t n_ref, int payload, int extra, HostColumns (*alloc)(void*, int64_t), void* sink,
                                 DeviceDecodeResult* res, int64_t* bad_job, int64_t* bad_record, char* err256) {
  if (!(payload == 2 && !extra && n_segs == 1 && segs[0].job_lo < segs[0].job_hi && segs[0].job_hi <= n_jobs)) return kStreamFallback;
  const size_t nb = segs[0].job_hi - segs[0].job_lo;
  size_t group = 0;
  int slots = 3;
  const char* on = getenv("MIDAS_SNPS_DECODE_STREAM");
  if (!on || atoi(on) != 0) {
    // (half a device-fill of the decoder's workgroups a group: two groups' kernels run side by side, on alternating streams)
    group = (size_t)std::max(64ll, bgzf_inflate_wave_blocks(ctx->prop.multiProcessorCount) / 2);
    if (const char* e = getenv("MIDAS_SNPS_DECODE_GROUP_BLOCKS")) group = (size_t)std::max(1ll, atoll(e));
    if (const char* e = getenv("MIDAS_SNPS_DECODE_SLOT_MB")) {        // a slot is ~2.5 x its blocks' inflated bytes (<= 64 KiB each)
      const size_t cap_blocks = (size_t)std::max(16ll, atoll(e) * (1ll << 20) / (160ll << 10));
      group = std::min(group, cap_blocks);
    }
    if (const char* e = getenv("MIDAS_SNPS_DECODE_SLOTS")) slots = std::max(1, std::min(4, atoi(e)));
  }
  if (!group || nb <= group + group / 4) return kStreamFallback;
  const size_t K = (nb + group - 1) / group;
  group = (nb + K - 1) / K;        // (equal groups, none above a wave)
  const int32_t sst = device_decode_stream(ctx, comp_base, jobs, segs[0], group, slots, ref_lens, n_ref, alloc, sink, res, bad_job, bad_record, err256);
  if (sst != kStreamFallback) return sst;
  if (getenv("MIDAS_SNPS_TRACE")) fprintf(stderr, "[device decode] streamed decode gave up (a record longer than what a group keeps behind its end): one arena\n");
  *bad_job = -1;
  *bad_record = -1;
  return kStreamFallback;
}

// DeviceDecoder::run (hostio.h): BGZF blocks of a BAM -- the whole file's, a rank's slice, or the runs that hold a rank's contigs --
// decoded on the device: up, inflated, resolved and CRC-checked (bgzf_inflate.hip), records found and decoded (bam_walk.hip), SEQ /
// QUAL / CIGAR cut out where the stream lies; the small columns are all that comes down.
// payload == 3 (midas_genes_count_bam; sink: its GenesBamCall, alloc and res unused): the same steps up to every kept record's
// offset, then the genes count over the records where they lie (genes_count.hip) -- no columns, no scans, no payload cut, and
// nothing per read comes down.
int32_t device_decode_run(void* user, const uint8_t* comp_base, const InflateJob* jobs, size_t n_jobs, uint64_t total, DecodeSegment* segs,
                          size_t n_segs, const int64_t* ref_lens, int32_t n_ref, int payload, int extra, HostColumns (*alloc)(void*, int64_t),
                          void* sink, DeviceDecodeResult* res, int64_t* bad_job, int64_t* bad_record, char* err256) {
  midas_snps_ctx* ctx = static_cast<midas_snps_ctx*>(user);
  *bad_job = -1;
  *bad_record = -1;
  std::lock_guard<std::mutex> g(ctx->device_mutex);
  Lap lap{"device decode", 30};
  TRY(kDecode, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const int32_t sst = decode_streamed_if_large(ctx, comp_base, jobs, n_jobs, segs, n_segs, ref_lens, n_ref, payload, extra, alloc, sink, res, bad_job, bad_record, err256);
  if (sst != kStreamFallback) return sst;
  // ---- the compressed bytes: every segment's blocks are consecutive in the file, the segments go up back to back ----------
  std::vector<size_t> seg_at(n_segs + 1, 0);      // where segment k's bytes start in the device's copy
  for (size_t k = 0; k < n_segs; ++k) {
    const DecodeSegment& sg = segs[k];
    if (sg.job_lo >= sg.job_hi || sg.job_hi > n_jobs) { if (err256) snprintf(err256, 256, "device decode: empty segment"); return MIDAS_SNPS_ERR_INVALID_ARG; }
    const size_t bytes = (size_t)(jobs[sg.job_hi - 1].cpos + jobs[sg.job_hi - 1].clen + 8 - jobs[sg.job_lo].cpos);
    seg_at[k + 1] = seg_at[k] + bytes;
  }
  const size_t comp_bytes = seg_at[n_segs];
  // ---- the arena (decode_plan.h InflateLayout); the columns are laid over everything behind the inflated bytes --------------------
  std::vector<InflateBlock> blocks(n_jobs);
  std::vector<uint32_t> want(n_jobs);
  unsigned long long n_match_room = 0;
  for (size_t k = 0; k < n_segs; ++k) {
    const uint64_t c0 = jobs[segs[k].job_lo].cpos;
    for (size_t j = segs[k].job_lo; j < segs[k].job_hi; ++j) {
      if (jobs[j].upos + jobs[j].ulen > total || jobs[j].cpos < c0) {
        if (err256) snprintf(err256, 256, "device decode: block %lld lies outside the buffers", (long long)j);
        return MIDAS_SNPS_ERR_INVALID_ARG;
      }
    }
    const size_t lo = segs[k].job_lo;
    fill_inflate_blocks(jobs + lo, segs[k].job_hi - lo, c0, seg_at[k], 0, blocks.data() + lo, want.data() + lo, &n_match_room);
  }
  const InflateLayout L((size_t)total, comp_bytes, n_jobs, (size_t)n_match_room);
  GenesBamCall* const genes = payload == 3 ? static_cast<GenesBamCall*>(sink) : nullptr;
  // (a BAM's columns are ~0.95 of its inflated bytes, the offsets and small columns ~0.2: the scratch must hold them too; the
  // genes count wants 40 bytes a record and 44 a gene instead)
  const size_t arena_bytes = std::max(L.end, L.at_comp + (size_t)total + (size_t)total / 3 + ((size_t)16 << 20)) + (genes ? (size_t)(n_ref > 0 ? n_ref : 0) * 64 : 0);
  bool pooled = false;
  void* arena_p = ctx->arena->take(arena_bytes, &pooled);
  if (!arena_p) { if (err256) snprintf(err256, 256, "device decode: out of device memory (%.1f GB)", (double)arena_bytes / 1e9); return MIDAS_SNPS_ERR_OUT_OF_MEMORY; }
  Loan loan{ctx->arena, arena_p};
  uint8_t* const base = static_cast<uint8_t*>(arena_p);
  lap("arena");
  // ---- blocks up, inflate, resolve, check ------------------------------------------------------------------------------------
  TRY(kDecode, hipMemcpyAsync(base + L.at_blocks, blocks.data(), n_jobs * sizeof(InflateBlock), hipMemcpyHostToDevice, s));
  TRY(kDecode, hipMemcpyAsync(base + L.at_crc, want.data(), n_jobs * 4, hipMemcpyHostToDevice, s));
  TRY(kDecode, hipMemsetAsync(base + L.at_comp + comp_bytes, 0, 512, s));
  const InflateParams ip = inflate_params(L, base, n_jobs);
  // (Inflating a first group of blocks while the next group's bytes go up -- four groups, a stream each -- was built and
  // measured: 216 ms against 188 ms for the whole decode of configs[2]'s BAM on the same box.  The copy threads and the
  // link are slowed by the running kernels by more than the overlap wins.  One upload, one launch.)
  const auto t_up = Clock::now();
  for (size_t k = 0; k < n_segs; ++k) {
    const int32_t cst = copy_to_device_staged(ctx, base + L.at_comp + seg_at[k], comp_base + jobs[segs[k].job_lo].cpos, seg_at[k + 1] - seg_at[k], s);
    if (cst != MIDAS_SNPS_OK) { if (err256) snprintf(err256, 256, "device decode: blocks to the device: %s", ctx->error_text().c_str()); return cst; }
  }
  if (genes) {       // (its laps: the upload by the host's clock, waited for; everything behind it between events)
    TRY(kGenes, hipStreamSynchronize(s));
    genes->ms[0] = (float)ms_since(t_up);
    TRY(kGenes, hipEventRecord(genes->ev[0], s));
  }
  if (lap.on) {      // (phase by phase, each waited for)
    TRY(kDecode, hipStreamSynchronize(s)); lap("blocks up");
    TRY(kDecode, launch_bgzf_inflate(ip, s, 1)); TRY(kDecode, hipStreamSynchronize(s)); lap("  inflate kernel");
    TRY(kDecode, launch_bgzf_inflate(ip, s, 2 | 8)); TRY(kDecode, hipStreamSynchronize(s)); lap("  resolve kernel");
    TRY(kDecode, launch_bgzf_inflate(ip, s, 4)); TRY(kDecode, hipStreamSynchronize(s)); lap("  crc kernel");
  } else {
    TRY(kDecode, launch_bgzf_inflate(ip, s));
  }
  std::vector<uint32_t> status(n_jobs);
  TRY(kDecode, hipMemcpyAsync(status.data(), ip.status, n_jobs * 4, hipMemcpyDeviceToHost, s));
  TRY(kDecode, hipStreamSynchronize(s));
  lap("blocks up, inflate, resolve, crc");
  bool again = false;
  const int32_t ast = inflate_again(kDecode, ip, blocks.data(), want.data(), status, s, &again, err256);
  if (ast != MIDAS_SNPS_OK) return ast;
  if (again) lap("streams decoded again");
  if (check_block_statuses(status, 0, bad_job, err256) != MIDAS_SNPS_OK) return MIDAS_SNPS_ERR_BAD_LAYOUT;
  if (genes) TRY(kGenes, hipEventRecord(genes->ev[1], s));
  // ---- the record walk: chunks of at most 32 KiB, laid out segment by segment over [from, stop) ---------------------------
  WalkTables walk{kDecode, err256};
  std::vector<size_t> seg_chunk(n_segs + 1, 0);
  for (size_t k = 0; k < n_segs; ++k) {
    const DecodeSegment& sg = segs[k];
    const unsigned long long limit = jobs[sg.job_hi - 1].upos + jobs[sg.job_hi - 1].ulen;
    walk.h.add_segment(sg.from, sg.stop < limit ? sg.stop : limit, limit, sg.exact != 0);
    seg_chunk[k + 1] = walk.h.size();
  }
  Scratch sc{base + L.at_comp, arena_bytes - L.at_comp};
  if (!walk.carve(sc, base, n_ref)) { if (err256) snprintf(err256, 256, "device decode: the arena is too small for the walk"); return MIDAS_SNPS_ERR_OUT_OF_MEMORY; }
  const int32_t walked = walk.walk(ref_lens, s);
  if (walked != MIDAS_SNPS_OK) return walked;
  lap("walk (guesses)");
  // stitch every segment in order; a chunk whose guess the chain does not hit is walked again from where the chain stands
  int rounds = 0;
  for (size_t k = 0; k < n_segs; ++k) {
    DecodeSegment& sg = segs[k];
    int32_t again_st = MIDAS_SNPS_OK;
    const StitchResult r = stitch_chunks(walk.h, seg_chunk[k], seg_chunk[k + 1], sg.exact ? sg.from : kNoOffset, &rounds,
                                         [&](size_t c, unsigned long long at) { again_st = walk.walk_again(c, at, s); return again_st == MIDAS_SNPS_OK; });
    if (r.what == Stitch::bad_chunk) { *bad_record = -2; return MIDAS_SNPS_ERR_BAD_LAYOUT; }
    if (r.what == Stitch::unsettled) { if (err256) snprintf(err256, 256, "device decode: the record boundaries did not settle"); return MIDAS_SNPS_ERR_UNSUPPORTED; }
    if (r.what == Stitch::failed) return again_st;
    const unsigned long long limit = jobs[sg.job_hi - 1].upos + jobs[sg.job_hi - 1].ulen;
    sg.first = r.first; sg.n_records = r.n_records; sg.n_unmapped = r.n_unmapped; sg.first_unmapped = r.first_unmapped;
    sg.end = r.end != kNoOffset ? r.end : (sg.stop < limit ? sg.stop : limit);
  }
  if (rounds && lap.on) fprintf(stderr, "[device decode] %d chunk(s) walked again\n", rounds);
  const long long n = (long long)walk.h.count_records();
  const int32_t up_st = walk.settled_up(s);
  if (up_st != MIDAS_SNPS_OK) return up_st;
  lap("stitch");
  const size_t n1 = (size_t)n + 1;
  unsigned long long* d_rec = sc.as<unsigned long long>(n1 * 8);
  if (genes) {
    if (!d_rec) { if (err256) snprintf(err256, 256, "genes count over a BAM: the arena is too small for the record offsets"); return MIDAS_SNPS_ERR_OUT_OF_MEMORY; }
    TRY(kGenes, launch_bam_offsets(walk.wp, walk.d_base, d_rec, s));
    TRY(kGenes, hipEventRecord(genes->ev[2], s));
    int64_t dropped = 0;
    for (size_t k = 0; k < n_segs; ++k) dropped += segs[k].n_unmapped;
    const int64_t stats[8] = {(int64_t)n, dropped, (int64_t)n_jobs, (int64_t)total, (int64_t)walk.h.size(), (int64_t)rounds, 0, 0};
    memcpy(genes->stats, stats, sizeof stats);
    const int32_t gst = genes_count_stream(ctx, base, (unsigned long long)total, d_rec, n, sc.p + sc.at, sc.bytes - sc.at, genes);
    if (gst != MIDAS_SNPS_OK && err256) snprintf(err256, 256, "%s", ctx->error_text().c_str());
    lap("genes: facts, filter, sort, sums");
    return gst;
  }
  BamColumnsParams cp;
  cp.d = base; cp.rec_off = d_rec; cp.n = n; cp.n_ref = n_ref;
  cp.refid = sc.as<int32_t>(n1 * 4); cp.pos = sc.as<int32_t>(n1 * 4);
  cp.nm = sc.as<int32_t>(n1 * 4); cp.l_seq = sc.as<int32_t>(n1 * 4);
  cp.mapq = sc.take(n1); cp.flag = sc.as<uint16_t>(n1 * 2);
  cp.seq_off = sc.as<long long>(n1 * 8); cp.qual_off = sc.as<long long>(n1 * 8);
  cp.cigar_off = sc.as<long long>(n1 * 8);
  cp.span = extra ? sc.as<int32_t>(n1 * 4) : nullptr;
  cp.unit_off = payload == 2 ? sc.as<long long>(n1 * 8) : nullptr;
  cp.bad_record = sc.as<unsigned long long>(8);
  long long* d_scan = sc.as<long long>(bam_scan_scratch_bytes(n));
  if (!d_scan) { if (err256) snprintf(err256, 256, "device decode: the arena is too small for the columns"); return MIDAS_SNPS_ERR_OUT_OF_MEMORY; }
  unsigned long long h_bad_record = kNoOffset;
  long long ends[4] = {0, 0, 0, 0};
  const int32_t col_st = run_columns(walk, d_rec, cp, d_scan, s, &h_bad_record, ends);
  if (col_st != MIDAS_SNPS_OK) return col_st;
  lap("offsets, columns, scans");
  if (h_bad_record != kNoOffset) { *bad_record = (int64_t)h_bad_record; return MIDAS_SNPS_ERR_BAD_LAYOUT; }
  const int64_t sb = ends[0], qb = ends[1], nc = ends[2];
  if (payload == 2) {
    // ---- resident: the records in the pileup kernel's own layout, ONE copy of every record's [cigar][seq][qual] run; every
    // column stays where it was decoded and only refID comes down (the host groups the records by contig with it) -------------
    const unsigned long long units = (unsigned long long)ends[3];
    if (units > kMaxDirectPayloadUnits) {
      if (err256) snprintf(err256, 256, "device decode: %llu bytes of read payload exceed the 32 GiB the direct layout addresses", units * 8ull);
      return MIDAS_SNPS_ERR_UNSUPPORTED;
    }
    DirectRec* d_drec = sc.as<DirectRec>((n1 + 1) * sizeof(DirectRec));
    uint8_t* d_pay = sc.take((size_t)units * 8 + 64);
    if (!d_pay) { if (err256) snprintf(err256, 256, "device decode: the arena is too small for the direct layout"); return MIDAS_SNPS_ERR_OUT_OF_MEMORY; }
    TRY(kDecode, hipMemsetAsync(d_pay + (size_t)units * 8, 0, 64, s));       // (a lane's 16-byte loads may overhang the last read)
    // (the inflated stream stays: raw columns are cut out of it, the side buffer only collects the producer's flags)
    DenseSide* d_side = sc.as<DenseSide>(sizeof(DenseSide));
    if (!d_side) { if (err256) snprintf(err256, 256, "device decode: the arena is too small for the direct layout"); return MIDAS_SNPS_ERR_OUT_OF_MEMORY; }
    TRY(kDecode, hipMemsetAsync(d_side, 0, sizeof(DenseSide), s));
    BamDirectParams dp;
    dp.stream = base; dp.rec_off = d_rec; dp.n_records = n;
    dp.pos = cp.pos; dp.nm = cp.nm; dp.unit_off = cp.unit_off;
    dp.rec = d_drec; dp.payload = d_pay;
    dp.side = d_side; dp.read_base = 0; dp.side_copy = 0;
    TRY(kDecode, launch_bam_direct(dp, ctx->prop.multiProcessorCount, s));
    DenseSide h_side{};
    TRY(kDecode, hipMemcpyAsync(&h_side, d_side, sizeof h_side, hipMemcpyDeviceToHost, s));
    const HostColumns hc = alloc(sink, n);
    if (!hc.refid) { TRY(kDecode, hipStreamSynchronize(s)); return MIDAS_SNPS_OK; }      // (the caller reports its own out-of-memory)
    if (n > 0) {
      const int32_t dst = copy_to_host(ctx, hc.refid, cp.refid, (size_t)n * 4);
      if (dst != MIDAS_SNPS_OK) { if (err256) snprintf(err256, 256, "device decode: columns to host: %s", ctx->error_text().c_str()); return dst; }
    }
    TRY(kDecode, hipStreamSynchronize(s));
    lap("direct layout, refID down");
    res->n_records = n; res->seq_bytes = sb; res->qual_bytes = qb; res->n_cigar = nc;
    ResidentReads& rr = res->resident;
    rr.rec = d_drec; rr.payload = d_pay; rr.refid = cp.refid; rr.pos = cp.pos; rr.nm = cp.nm; rr.l_seq = cp.l_seq; rr.mapq = cp.mapq; rr.flag = cp.flag;
    rr.seq_off = reinterpret_cast<int64_t*>(cp.seq_off); rr.qual_off = reinterpret_cast<int64_t*>(cp.qual_off);
    rr.cigar_off = reinterpret_cast<int64_t*>(cp.cigar_off); rr.unit_off = reinterpret_cast<int64_t*>(cp.unit_off);
    rr.stream = base; rr.rec_off = reinterpret_cast<const uint64_t*>(d_rec);
    rr.payload_units = (int64_t)units;
    rr.dense_flags = h_side.flags;
    res->dev_owner = new ArenaLoan{loan.pool, loan.p};       // everything lives in the arena: it stays lent until the handle is closed
    res->dev_free = arena_loan_free;
    loan.p = nullptr;
    return MIDAS_SNPS_OK;
  }
  // ---- SEQ / QUAL / CIGAR cut out of the stream, behind everything taken so far ---------------------------------------------
  uint8_t *d_seq = nullptr, *d_qual = nullptr, *d_cig = nullptr;
  DeviceBuf own;
  if (payload) {
    d_seq = sc.take((size_t)sb + 64);
    d_qual = sc.take((size_t)qb + 64);
    d_cig = sc.take((size_t)nc * 4 + 64);
    if (!d_cig) {       // (the scratch cannot hold them: a buffer of their own)
      const size_t need = round256((size_t)sb + 64) + round256((size_t)qb + 64) + round256((size_t)nc * 4 + 64);
      TRY(kDecode, hipMalloc(&own.p, need));
      d_seq = static_cast<uint8_t*>(own.p);
      d_qual = d_seq + round256((size_t)sb + 64);
      d_cig = d_qual + round256((size_t)qb + 64);
    }
    TRY(kDecode, hipMemsetAsync(d_cig + (size_t)nc * 4, 0, 64, s));
    PayloadParams pp;
    pp.stream = base;
    pp.rec_off = d_rec;
    pp.n_records = n;
    pp.seq_off = cp.seq_off; pp.qual_off = cp.qual_off; pp.cigar_off = cp.cigar_off;
    pp.seq4 = d_seq; pp.qual = d_qual; pp.cigar = reinterpret_cast<uint32_t*>(d_cig);
    // (Launched on a stream of its own so that the small columns go down the link while it runs: measured, 24.5 ms against
    // 20.3 ms one behind the other -- the copy kernels and this one slow each other by more than the overlap wins.)
    TRY(kDecode, launch_bam_payload(pp, ctx->prop.multiProcessorCount, s));
  }
  // ---- the small columns down ---------------------------------------------------------------------------------------------
  const HostColumns hc = alloc(sink, n);
  if (!hc.cigar_off) { TRY(kDecode, hipStreamSynchronize(s)); return MIDAS_SNPS_OK; }      // (the caller reports its own out-of-memory)
  const std::pair<void*, std::pair<const void*, size_t>> cols[] = {
      {hc.refid, {cp.refid, (size_t)n * 4}}, {hc.pos, {cp.pos, (size_t)n * 4}}, {hc.nm, {cp.nm, (size_t)n * 4}}, {hc.l_seq, {cp.l_seq, (size_t)n * 4}},
      {hc.mapq, {cp.mapq, (size_t)n}}, {hc.flag, {cp.flag, (size_t)n * 2}}, {hc.seq_off, {cp.seq_off, n1 * 8}}, {hc.qual_off, {cp.qual_off, n1 * 8}},
      {hc.cigar_off, {cp.cigar_off, n1 * 8}}, {extra ? hc.span : nullptr, {cp.span, (size_t)n * 4}}, {extra ? hc.rec_off : nullptr, {d_rec, (size_t)n * 8}}};
  for (const auto& c : cols) {
    const int32_t st = c.second.second && c.first ? copy_to_host(ctx, c.first, c.second.first, c.second.second) : MIDAS_SNPS_OK;
    if (st != MIDAS_SNPS_OK) { if (err256) snprintf(err256, 256, "device decode: columns to host: %s", ctx->error_text().c_str()); return st; }
  }
  TRY(kDecode, hipStreamSynchronize(s));
  lap("payload cut, small columns down");
  res->n_records = n; res->seq_bytes = sb; res->qual_bytes = qb; res->n_cigar = nc;
  res->dev_seq = d_seq; res->dev_qual = d_qual; res->dev_cigar = d_cig;
  if (!payload) return MIDAS_SNPS_OK;       // (the arena goes back with `loan`)
  if (own.p) {        // the columns have a buffer of their own: the arena goes back now
    res->dev_owner = own.p;
    res->dev_free = device_free;
    own.p = nullptr;
  } else {            // the columns live in the arena: it stays lent until the handle is closed
    // (and with them the small columns the host has just been given: a batch made from those host arrays need not send them up
    // again -- midas_arena_pool::find_twin, midas_snps_batch_create)
    for (const auto& c : cols)
      if (c.first && c.second.first != static_cast<const void*>(d_rec)) loan.pool->add_twin(c.first, c.second.first, c.second.second, loan.p);
    res->dev_owner = new ArenaLoan{loan.pool, loan.p};
    res->dev_free = arena_loan_free;
    loan.p = nullptr;
  }
  return MIDAS_SNPS_OK;
}
}  // namespace

extern "C" {

int32_t midas_snps_inflate_blocks(midas_snps_ctx* ctx, const uint8_t* comp, int64_t comp_bytes, int64_t n_blocks,
                                  const int64_t* cpos, const int32_t* clen, const int64_t* upos, const int32_t* ulen,
                                  const uint32_t* crc, uint8_t* out, int64_t out_bytes, int64_t* bad_block) {
  if (!ctx || comp_bytes < 0 || n_blocks < 0 || out_bytes < 0 || (n_blocks > 0 && (!comp || !cpos || !clen || !upos || !ulen || !out)))
    return MIDAS_SNPS_ERR_INVALID_ARG;
  std::vector<InflateJob> jobs((size_t)n_blocks);
  for (int64_t k = 0; k < n_blocks; ++k) {
    if (cpos[k] < 0 || clen[k] < 0 || upos[k] < 0 || ulen[k] < 0) return fail(ctx, MIDAS_SNPS_ERR_INVALID_ARG, "inflate_blocks: negative offset or size");
    jobs[(size_t)k] = InflateJob{(uint64_t)cpos[k], (uint64_t)upos[k], (uint32_t)clen[k], (uint32_t)ulen[k], crc ? crc[k] : 0u, crc ? 1u : 0u};
  }
  const InflateSegment seg{comp, (size_t)comp_bytes};
  char err[256] = {0};
  InflateUser iu{ctx};
  const int32_t st = device_inflate(&iu, &seg, 1, jobs.data(), jobs.size(), out, (size_t)out_bytes, bad_block, err);
  if (st != MIDAS_SNPS_OK) return fail(ctx, st, err);
  return MIDAS_SNPS_OK;
}

int32_t midas_bam_open_device(const char* path, midas_snps_ctx* ctx, midas_bam** out, char* err256) {
  if (!ctx) return MIDAS_SNPS_ERR_INVALID_ARG;
  InflateUser iu{ctx};
  const BlockInflater inf{&iu, device_inflate};
  return bam_open_with(path, &inf, out, err256);
}

int32_t midas_bam_load_device(const char* path, midas_snps_ctx* ctx, midas_bam** out, int64_t* n_reads, int64_t* seq_bytes,
                              int64_t* qual_bytes, int64_t* n_cigar, char* err256) {
  if (!ctx || !path || !out) return MIDAS_SNPS_ERR_INVALID_ARG;
  const DeviceDecoder dec{ctx, device_decode_run};
  const int32_t st = bam_decode_on_device(path, &dec, out, n_reads, seq_bytes, qual_bytes, n_cigar, err256);
  if (st != MIDAS_SNPS_ERR_UNSUPPORTED) return st;
  return bam_load_device_host_walk(path, ctx, out, n_reads, seq_bytes, qual_bytes, n_cigar, err256);      // (boundaries not settled: the host walks)
}

int32_t midas_bam_load_resident(const char* path, midas_snps_ctx* ctx, midas_bam** out, int64_t* n_reads, int64_t* sum_l_seq, char* err256) {
  if (!ctx || !path || !out) return MIDAS_SNPS_ERR_INVALID_ARG;
  const DeviceDecoder dec{ctx, device_decode_run};
  int64_t qb = 0;
  const int32_t st = bam_decode_on_device(path, &dec, out, n_reads, nullptr, &qb, nullptr, err256, 2);
  if (sum_l_seq) *sum_l_seq = qb;       // (QUAL holds one byte per base)
  return st;
}

int32_t midas_bam_load_ranges_resident(midas_bam* bam, midas_snps_ctx* ctx, int32_t n_ranges, const int64_t* range_begin,
                                       const int64_t* range_end, int64_t* n_reads, int64_t* sum_l_seq, char* err256) {
  if (!bam || !ctx) return MIDAS_SNPS_ERR_INVALID_ARG;
  const DeviceDecoder dec{ctx, device_decode_run};
  int64_t qb = 0;
  const int32_t st = bam_load_ranges_on_device(bam, &dec, n_ranges, range_begin, range_end, n_reads, nullptr, &qb, nullptr, err256, 2);
  if (sum_l_seq) *sum_l_seq = qb;
  return st;
}

int32_t midas_bam_is_resident(const midas_bam* bam) { return bam_resident(bam, nullptr, nullptr, nullptr, nullptr) ? 1 : 0; }

// The fall-back of a resident handle: the three payload columns cut out of the inflated stream it still holds (a buffer of
// their own), the small columns brought down -- afterwards the handle answers midas_bam_columns as after midas_bam_load_device.
int32_t midas_bam_resident_to_columns(midas_bam* bam, midas_snps_ctx* ctx, int64_t* seq_bytes, int64_t* qual_bytes, int64_t* n_cigar, char* err256) {
  if (!bam || !ctx) return MIDAS_SNPS_ERR_INVALID_ARG;
  int64_t n = 0, sb = 0, qb = 0, nc = 0;
  const midas::ResidentReads* rr = bam_resident(bam, &n, &sb, &qb, &nc);
  if (!rr) { if (err256) snprintf(err256, 256, "the BAM handle holds no device-resident records"); return MIDAS_SNPS_ERR_INVALID_ARG; }
  if (seq_bytes) *seq_bytes = sb;
  if (qual_bytes) *qual_bytes = qb;
  if (n_cigar) *n_cigar = nc;
  if (midas_bam_payload_on_device(bam)) return MIDAS_SNPS_OK;         // (done before)
  std::lock_guard<std::mutex> g(ctx->device_mutex);
  TRY(kToColumns, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const size_t at_q = round256((size_t)sb + 64), at_c = at_q + round256((size_t)qb + 64), bytes = at_c + round256((size_t)nc * 4 + 64);
  DeviceBuf own;
  TRY(kToColumns, hipMalloc(&own.p, bytes));
  uint8_t* base = static_cast<uint8_t*>(own.p);
  TRY(kToColumns, hipMemsetAsync(base + sb, 0, 64, s));
  TRY(kToColumns, hipMemsetAsync(base + at_q + qb, 0, 64, s));
  TRY(kToColumns, hipMemsetAsync(base + at_c + (size_t)nc * 4, 0, 64, s));
  PayloadParams pp;
  pp.stream = rr->stream;
  pp.rec_off = reinterpret_cast<const unsigned long long*>(rr->rec_off);
  if (!rr->stream) {      // (a streamed decode: out of the direct layout, the side buffer's exact copies over the decoded bytes)
    pp.stream = rr->payload; pp.drec = static_cast<const DirectRec*>(rr->rec);
    pp.side = static_cast<const DenseSide*>(rr->side); pp.side_first = 0;
  }
  pp.n_records = n;
  pp.seq_off = reinterpret_cast<const long long*>(rr->seq_off); pp.qual_off = reinterpret_cast<const long long*>(rr->qual_off);
  pp.cigar_off = reinterpret_cast<const long long*>(rr->cigar_off);
  pp.seq4 = base; pp.qual = base + at_q; pp.cigar = reinterpret_cast<uint32_t*>(base + at_c);
  TRY(kToColumns, launch_bam_payload(pp, ctx->prop.multiProcessorCount, s));
  HostColumns hc{};
  if (!bam_alloc_host_columns(bam, n, &hc)) { if (err256) snprintf(err256, 256, "resident BAM to columns: out of host memory"); return MIDAS_SNPS_ERR_OUT_OF_MEMORY; }
  const size_t n1 = (size_t)n + 1;
  const std::pair<void*, std::pair<const void*, size_t>> cols[] = {
      {hc.pos, {rr->pos, (size_t)n * 4}}, {hc.nm, {rr->nm, (size_t)n * 4}}, {hc.l_seq, {rr->l_seq, (size_t)n * 4}}, {hc.mapq, {rr->mapq, (size_t)n}},
      {hc.flag, {rr->flag, (size_t)n * 2}}, {hc.seq_off, {rr->seq_off, n1 * 8}}, {hc.qual_off, {rr->qual_off, n1 * 8}}, {hc.cigar_off, {rr->cigar_off, n1 * 8}}};
  for (const auto& c : cols) {
    if (!c.second.second) continue;
    const int32_t st = copy_to_host(ctx, c.first, c.second.first, c.second.second);
    if (st != MIDAS_SNPS_OK) { if (err256) snprintf(err256, 256, "resident BAM to columns: %s", ctx->error_text().c_str()); return st; }
  }
  // (refID is in the handle's host memory already, and stays there: the caller holds views of it)
  TRY(kToColumns, hipStreamSynchronize(s));
  bam_resident_became_columns(bam, base, base + at_q, base + at_c, own.p, device_free);
  own.p = nullptr;
  return MIDAS_SNPS_OK;
}

int32_t midas_genes_count_bam(midas_snps_ctx* ctx, midas_bam* bam, const midas_snps_thresholds* thr, int64_t n_genes, const int64_t* gene_length,
                              int64_t* out_aligned, int64_t* out_mapped, double* out_depth, int64_t* out_stats8, float* out_ms8, char* err256) {
  if (!ctx || !bam || !thr || n_genes < 0 || (n_genes > 0 && (!gene_length || !out_aligned || !out_mapped || !out_depth))) return MIDAS_SNPS_ERR_INVALID_ARG;
  ctx->clear_error();
  ctx->err_read = -1;
  if (err256) err256[0] = 0;
  if (n_genes != (int64_t)midas_bam_n_refs(bam)) {
    if (err256) snprintf(err256, 256, "genes count over a BAM: %lld gene lengths for the %d references of the header", (long long)n_genes, midas_bam_n_refs(bam));
    return fail(ctx, MIDAS_SNPS_ERR_INVALID_ARG, err256 ? err256 : "");
  }
  GenesBamCall call;
  call.thr = thr; call.n_genes = n_genes; call.gene_length = gene_length;
  call.out_aligned = out_aligned; call.out_mapped = out_mapped; call.out_depth = out_depth;
  struct Events { GenesBamCall& c; ~Events() { for (hipEvent_t e : c.ev) if (e) (void)hipEventDestroy(e); } } events{call};
  TRY(kGenes, hipSetDevice(ctx->device));
  for (hipEvent_t& e : call.ev) TRY(kGenes, hipEventCreate(&e));
  char text[256] = {0};
  const DeviceDecoder dec{ctx, device_decode_run};
  const int32_t st = bam_genes_on_device(bam, &dec, &call, text);
  if (out_stats8) memcpy(out_stats8, call.stats, sizeof call.stats);
  if (out_ms8) memcpy(out_ms8, call.ms, sizeof call.ms);
  if (st != MIDAS_SNPS_OK) {
    if (err256) snprintf(err256, 256, "%s", text);
    if (ctx->error_text().empty()) ctx->set_error(text);       // (a status of the decode: the context says what the buffer says)
  }
  return st;
}

int32_t midas_bam_load_ranges_device(midas_bam* bam, midas_snps_ctx* ctx, int32_t n_ranges, const int64_t* range_begin,
                                     const int64_t* range_end, int64_t* n_reads, int64_t* seq_bytes, int64_t* qual_bytes,
                                     int64_t* n_cigar, char* err256) {
  if (!ctx) return MIDAS_SNPS_ERR_INVALID_ARG;
  const DeviceDecoder dec{ctx, device_decode_run};
  const int32_t st = bam_load_ranges_on_device(bam, &dec, n_ranges, range_begin, range_end, n_reads, seq_bytes, qual_bytes, n_cigar, err256);
  if (st != MIDAS_SNPS_ERR_UNSUPPORTED) return st;
  InflateUser iu{ctx};       // (boundaries not settled on the device: its inflater, the host's walk)
  const BlockInflater inf{&iu, device_inflate};
  return bam_load_ranges_with(bam, &inf, n_ranges, range_begin, range_end, n_reads, seq_bytes, qual_bytes, n_cigar, err256);
}

int32_t midas_bam_open_slice_device(const char* path, int32_t slice, int32_t n_slices, midas_snps_ctx* ctx, midas_bam** out, char* err256) {
  if (!ctx) return MIDAS_SNPS_ERR_INVALID_ARG;
  const DeviceDecoder dec{ctx, device_decode_run};
  return bam_open_slice_with(path, slice, n_slices, &dec, out, err256);
}

}  // extern "C"
