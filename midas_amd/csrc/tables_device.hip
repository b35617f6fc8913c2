// The input end of merge_midas.py snps on the device, behind the C ABI: the samples' count tables as one resident set
// (midas_merge_tables_*), the samples' <species>.snps.gz inflated and parsed into it (midas_snps_tableset_read_counts_device), and the
// row parser on text of the caller's (midas_snps_parse_rows_device).
//
// read_counts_device: the gzip members that hold the wanted rows are chosen and cut into groups on the host (tables_plan.h);
// per group the members' compressed bytes go up on the copy stream -- one copy per run of neighbouring members of a file --
// while the group before is in the kernels: inflate + CRC-32 (bgzf_inflate.hip: a lane per member, checked against the trailer's
// CRC-32, the size against its ISIZE), line index, row parser (tables_scan.hip).  Nothing per site comes down: per member a
// status and a line count, per table the first malformed row.  Two slots of device memory, sized by the largest group.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>

#include "ctx_internal.h"
#include "kernels.h"
#include "hostio.h"
#include "decode_plan.h"
#include "tables_plan.h"

using namespace midas;
using namespace midas_ctx;

static_assert(sizeof(TableTextMember) == 48, "the slots lay out the member tables");

namespace {

constexpr char kWho[] = "device table read";
int32_t hip_err(char* err256, hipError_t e, const char* what) {
  if (err256) snprintf(err256, 256, "%s: %s: %s", kWho, what, hipGetErrorString(e));
  (void)hipGetLastError();
  return e == hipErrorOutOfMemory ? MIDAS_SNPS_ERR_OUT_OF_MEMORY : MIDAS_SNPS_ERR_HIP;
}
// (in a function that has `err256`)
#define TRY(call) do { const hipError_t e__ = (call); if (e__ != hipSuccess) return hip_err(err256, e__, #call); } while (0)

inline uint32_t rd32(const uint8_t* p) { uint32_t v; memcpy(&v, p, 4); return v; }

struct EventSet {      // (destroyed on every way out)
  hipEvent_t e[8] = {};
  ~EventSet() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
};

// The regions of a slot behind an inflate's (decode_plan.h InflateLayout): member table, line counts, scan scratch, line ends,
// lines per member.
struct SlotLayout {
  InflateLayout infl;
  size_t at_members, at_words, at_scan, at_ends, at_lines, end;
  SlotLayout(size_t text, size_t comp, size_t n, size_t room, size_t cap_lines) : infl(text, comp, n, room) {
    const size_t n16 = (text + 15) / 16;
    at_members = infl.end;
    at_words = at_members + round256(n * sizeof(TableTextMember));
    at_scan = at_words + round256((n16 + 1) * 4);
    at_ends = at_scan + round256(scan_scratch_words((long long)n16 + 1) * 4);
    at_lines = at_ends + round256(cap_lines * 4);
    end = at_lines + round256(n * 4);
  }
};

// One group on its way through a slot: what the host laid out for it.
struct GroupWork {
  std::vector<InflateBlock> blocks;
  std::vector<uint32_t> want;
  std::vector<TableTextMember> members;
  struct Run { const uint8_t* src; size_t n, at; };      // a run of a file's bytes -> the slot's compressed region
  std::vector<Run> runs;
  size_t text = 0, comp = 0, room = 0, cap_lines = 0;
  long long n_take = 0;
};

TablesScanParams scan_params(const SlotLayout& L, uint8_t* base, const GroupWork& w, uint32_t* counts, unsigned long long* bad) {
  TablesScanParams p;
  p.text = base;
  p.n16 = (long long)((w.text + 15) / 16);
  p.members = reinterpret_cast<const TableTextMember*>(base + L.at_members);
  p.n_members = (int)w.members.size();
  p.word_lines = reinterpret_cast<uint32_t*>(base + L.at_words);
  p.scan_scratch = reinterpret_cast<uint32_t*>(base + L.at_scan);
  p.line_end = reinterpret_cast<uint32_t*>(base + L.at_ends);
  p.cap_lines = (uint32_t)w.cap_lines;
  p.member_lines = reinterpret_cast<uint32_t*>(base + L.at_lines);
  p.counts = counts;
  p.bad = bad;
  p.n_take = w.n_take;
  return p;
}

InflateParams inflate_params_of(const InflateLayout& L, uint8_t* base, size_t n) {
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

// the cap on a group's inflated text: MIDAS_SNPS_MERGE_READ_KB, else a twelfth of the free device memory (a slot holds the text,
// the compressed bytes, the match lists and the line index: about three times the text; there are two) within [16 MiB, 3.5 GiB].
// As large as memory allows, because the inflater is latency-bound: a launch takes as long for one member as for ten thousand
// (measured: 75 ms a group of 2 940 members of 16 384 rows), so every further group costs a whole launch.  Text offsets are
// 32-bit: below 4 GiB.
uint64_t text_cap() {
  if (const char* e = getenv("MIDAS_SNPS_MERGE_READ_KB")) {
    const double v = atof(e);
    if (v > 0) return (uint64_t)(v * 1024.0);
  }
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); free_b = (size_t)4 << 30; }
  const uint64_t cap = free_b / 12;
  return std::min<uint64_t>(std::max<uint64_t>(cap, (uint64_t)16 << 20), (uint64_t)7 << 29);
}

}  // namespace

int32_t midas_ctx::merge_tables_from_host(midas_snps_ctx* ctx, int32_t n_samples, int64_t n_sites, const uint32_t* const* sample_counts,
                                          midas_merge_tables** out) {
  *out = nullptr;
  midas_merge_tables* t = nullptr;
  ST_TRY(midas_merge_tables_create(ctx, n_samples, n_sites, &t));
  for (int32_t s = 0; s < n_samples; ++s) {
    if (n_sites > 0 && !sample_counts[s]) { midas_merge_tables_free(t); return MIDAS_SNPS_ERR_INVALID_ARG; }
    const hipError_t e = n_sites > 0 ? hipMemcpyAsync(t->d + (size_t)s * (size_t)n_sites * 4, sample_counts[s], (size_t)n_sites * 16, hipMemcpyHostToDevice, ctx->stream)
                                     : hipSuccess;
    if (e != hipSuccess) { midas_merge_tables_free(t); return hip_fail(ctx, e, "merge tables: upload"); }
  }
  *out = t;
  return MIDAS_SNPS_OK;
}

extern "C" {

int32_t midas_merge_tables_create(midas_snps_ctx* ctx, int32_t n_samples, int64_t n_rows, midas_merge_tables** out) {
  if (!ctx || n_samples <= 0 || n_rows < 0 || !out) return MIDAS_SNPS_ERR_INVALID_ARG;
  *out = nullptr;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  midas_merge_tables* t = new (std::nothrow) midas_merge_tables();
  if (!t) return MIDAS_SNPS_ERR_OUT_OF_MEMORY;
  t->device = ctx->device; t->n_samples = n_samples; t->n_rows = n_rows;
  const hipError_t e = hipMalloc(reinterpret_cast<void**>(&t->d), std::max<size_t>((size_t)n_samples * (size_t)n_rows * 16, 16));
  if (e != hipSuccess) { delete t; return hip_fail(ctx, e, "merge tables: hipMalloc"); }
  *out = t;
  return MIDAS_SNPS_OK;
}

void midas_merge_tables_free(midas_merge_tables* t) {
  if (!t) return;
  if (t->d) (void)hipFree(t->d);
  delete t;
}

int32_t midas_merge_tables_shape(const midas_merge_tables* t, int32_t* n_samples, int64_t* n_rows) {
  if (!t) return MIDAS_SNPS_ERR_INVALID_ARG;
  if (n_samples) *n_samples = t->n_samples;
  if (n_rows) *n_rows = t->n_rows;
  return MIDAS_SNPS_OK;
}

int32_t midas_merge_tables_set_host(midas_snps_ctx* ctx, midas_merge_tables* t, int32_t sample, int64_t n_rows, const uint32_t* counts) {
  if (!ctx || !t || sample < 0 || sample >= t->n_samples || n_rows < 0 || n_rows > t->n_rows || (n_rows > 0 && !counts)) return MIDAS_SNPS_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> g(ctx->device_mutex);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (n_rows > 0) HIP_TRY(ctx, hipMemcpyAsync(t->d + (size_t)sample * (size_t)t->n_rows * 4, counts, (size_t)n_rows * 16, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return MIDAS_SNPS_OK;
}

int32_t midas_merge_tables_fetch(midas_snps_ctx* ctx, const midas_merge_tables* t, int32_t sample, int64_t n_rows, uint32_t* out) {
  if (!ctx || !t || sample < 0 || sample >= t->n_samples || n_rows < 0 || n_rows > t->n_rows || (n_rows > 0 && !out)) return MIDAS_SNPS_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> g(ctx->device_mutex);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (n_rows > 0) HIP_TRY(ctx, hipMemcpyAsync(out, t->d + (size_t)sample * (size_t)t->n_rows * 4, (size_t)n_rows * 16, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return MIDAS_SNPS_OK;
}

int32_t midas_snps_tableset_read_counts_device(midas_snps_ctx* ctx, midas_snps_tableset* ts, int64_t row_begin, int64_t n_rows, int32_t first_sample_slot,
                                               midas_merge_tables* tables, int64_t* out_stats8, float* out_ms4, char* err256) {
  if (!ctx || !ts || !tables || row_begin < 0 || n_rows < 0 || first_sample_slot < 0) return MIDAS_SNPS_ERR_INVALID_ARG;
  if (err256) err256[0] = 0;
  if (out_stats8) memset(out_stats8, 0, 8 * sizeof(int64_t));
  if (out_ms4) memset(out_ms4, 0, 4 * sizeof(float));
  const int32_t n_tables = tableset_tables(ts);
  if (first_sample_slot + n_tables > tables->n_samples) {
    if (err256) snprintf(err256, 256, "%s: %d tables from slot %d on do not fit a set of %d samples", kWho, n_tables, first_sample_slot, tables->n_samples);
    return MIDAS_SNPS_ERR_INVALID_ARG;
  }
  // ---- the plan --------------------------------------------------------------------------------------------------------------
  int64_t shortest = INT64_MAX;
  for (int32_t t = 0; t < n_tables; ++t) {
    const int64_t rows = tableset_rows(ts, t);
    if (rows < 0) {      // written by the reference (or round 1): the caller takes the host's readers
      if (err256) snprintf(err256, 256, "%s: the file does not announce its rows", tableset_path(ts, t));
      return MIDAS_SNPS_ERR_UNSUPPORTED;
    }
    shortest = std::min(shortest, rows);
  }
  const int64_t n = std::min(n_rows, std::max<int64_t>(0, shortest - row_begin));      // the zip over the tables stops at the shortest
  for (int32_t t = 0; t < n_tables; ++t) {      // (a range that begins behind a table's end: refused in the host reader's words)
    if (tableset_rows(ts, t) < row_begin + n) {
      if (err256) snprintf(err256, 256, "%s: rows up to %lld asked of a table that holds fewer (or does not say)", tableset_path(ts, t), (long long)(row_begin + n));
      return MIDAS_SNPS_ERR_INVALID_ARG;
    }
  }
  if (n > tables->n_rows) {
    if (err256) snprintf(err256, 256, "%s: %lld rows do not fit a set of %lld", kWho, (long long)n, (long long)tables->n_rows);
    return MIDAS_SNPS_ERR_INVALID_ARG;
  }
  std::vector<std::vector<TableMemberSpan>> spans((size_t)n_tables);
  std::vector<ChosenMember> chosen;
  for (int32_t t = 0; t < n_tables; ++t) {
    spans[(size_t)t] = tableset_members(ts, t);
    size_t file_bytes = 0;
    (void)tableset_file(ts, t, &file_bytes);
    for (const TableMemberSpan& m : spans[(size_t)t]) {      // (what the open found; held to the file all the same: the trailer is read below)
      if (m.data + (uint64_t)m.clen + 8u > file_bytes) {
        if (err256) snprintf(err256, 256, "%s: a member lies outside the file", tableset_path(ts, t));
        return MIDAS_SNPS_ERR_BAD_LAYOUT;
      }
    }
    const int64_t got = choose_members(spans[(size_t)t].data(), spans[(size_t)t].size(), t, row_begin, n, chosen);
    if (got != n) {
      if (err256) snprintf(err256, 256, "%s: %lld of the %lld rows asked for", tableset_path(ts, t), (long long)got, (long long)n);
      return MIDAS_SNPS_ERR_BAD_LAYOUT;
    }
  }
  if (out_stats8) { out_stats8[0] = n_tables; out_stats8[1] = (int64_t)chosen.size(); out_stats8[5] = n; }
  if (chosen.empty()) return MIDAS_SNPS_OK;
  std::lock_guard<std::mutex> g(ctx->device_mutex);
  TRY(hipSetDevice(ctx->device));
  const std::vector<MemberGroup> groups = group_members(chosen, spans, text_cap());
  // ---- every group laid out ---------------------------------------------------------------------------------------------------
  std::vector<GroupWork> work(groups.size());
  size_t slot_bytes = 0;
  for (size_t gi = 0; gi < groups.size(); ++gi) {
    const MemberGroup& G = groups[gi];
    GroupWork& w = work[gi];
    if (G.text >= ((uint64_t)1 << 32) - 64) {
      if (err256) snprintf(err256, 256, "%s: a gzip member of %llu bytes of text (offsets are 32-bit)", tableset_path(ts, chosen[G.lo].table), (unsigned long long)G.text);
      return MIDAS_SNPS_ERR_UNSUPPORTED;
    }
    unsigned long long room = 0;
    uint32_t text_at = 0, take_base = 0;
    for (size_t k = G.lo; k < G.hi; ++k) {
      const ChosenMember& c = chosen[k];
      const TableMemberSpan& m = spans[(size_t)c.table][(size_t)c.member];
      size_t file_bytes = 0;      // (every member was held to it above)
      const uint8_t* file = tableset_file(ts, c.table, &file_bytes);
      // neighbours in the file go up in one copy (the 36 bytes of trailer and header between them with them)
      const bool joins = k > G.lo && chosen[k - 1].table == c.table && chosen[k - 1].member + 1 == c.member;
      if (!joins) {
        w.comp = (w.comp + 15) & ~(size_t)15;
        w.runs.push_back(GroupWork::Run{file + m.data, 0, w.comp});
      }
      GroupWork::Run& run = w.runs.back();
      const size_t in_run = (size_t)((file + m.data) - run.src);
      run.n = in_run + m.clen;
      w.comp = run.at + run.n;
      const uint32_t cap = first_pass_room(m.ulen);
      w.blocks.push_back(InflateBlock{(unsigned long long)(run.at + in_run), (unsigned long long)text_at, room, m.clen, m.ulen, cap, 0u});
      w.want.push_back(rd32(file + m.data + m.clen));       // the trailer: CRC-32, then ISIZE (= ulen, which the inflate must reach exactly)
      room += cap;
      TableTextMember tm;
      tm.start = text_at; tm.ulen = m.ulen;
      tm.skip = (uint32_t)c.skip; tm.take = (uint32_t)c.take; tm.take_base = take_base;
      tm.table = (uint32_t)c.table; tm.header = c.header; tm.rows = (uint32_t)m.rows;
      tm.dst_row = (unsigned long long)(first_sample_slot + c.table) * (unsigned long long)tables->n_rows + (unsigned long long)c.out_row;
      int64_t row0 = 0;
      for (int32_t q = 0; q < c.member; ++q) row0 += spans[(size_t)c.table][(size_t)q].rows;
      tm.table_row = (unsigned long long)row0;
      w.members.push_back(tm);
      text_at += (uint32_t)member_text_room(m.ulen);
      take_base += (uint32_t)c.take;
      w.cap_lines += (size_t)m.rows + 1;
    }
    w.text = text_at; w.room = (size_t)room; w.n_take = take_base;
    const SlotLayout L(w.text, w.comp, w.members.size(), w.room, w.cap_lines);
    slot_bytes = std::max(slot_bytes, L.end);
  }
  // ---- two slots, the per-table results, the events ----------------------------------------------------------------------------
  DeviceBuf slot[2], d_bad;
  TRY(hipMalloc(&slot[0].p, slot_bytes));
  if (groups.size() > 1) TRY(hipMalloc(&slot[1].p, slot_bytes));
  TRY(hipMalloc(&d_bad.p, (size_t)n_tables * 8));
  hipStream_t s = ctx->stream;
  if (!ctx->copy_stream && hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); ctx->copy_stream = nullptr; }
  hipStream_t cs = ctx->copy_stream ? ctx->copy_stream : s;
  TRY(hipMemsetAsync(d_bad.p, 0xFF, (size_t)n_tables * 8, s));
  EventSet ev;      // 0, 1: a group's upload (copy stream); 2..5: around inflate + CRC, index, parse; 6: the upload has landed
  for (hipEvent_t& e : ev.e) TRY(hipEventCreate(&e));
  float ms[4] = {0.f, 0.f, 0.f, 0.f};
  int64_t again_total = 0, comp_total = 0, text_total = 0;
  auto upload = [&](size_t gi, char* err256) -> int32_t {      // group gi's bytes and tables into its slot, on the copy stream
    const GroupWork& w = work[gi];
    uint8_t* base = static_cast<uint8_t*>(slot[gi & 1].p);
    const SlotLayout L(w.text, w.comp, w.members.size(), w.room, w.cap_lines);
    TRY(hipEventRecord(ev.e[0], cs));
    for (const GroupWork::Run& r : w.runs) TRY(hipMemcpyAsync(base + L.infl.at_comp + r.at, r.src, r.n, hipMemcpyHostToDevice, cs));
    TRY(hipMemsetAsync(base + L.infl.at_comp + w.comp, 0, 512, cs));
    TRY(hipMemcpyAsync(base + L.infl.at_blocks, w.blocks.data(), w.blocks.size() * sizeof(InflateBlock), hipMemcpyHostToDevice, cs));
    TRY(hipMemcpyAsync(base + L.infl.at_crc, w.want.data(), w.want.size() * 4, hipMemcpyHostToDevice, cs));
    TRY(hipMemcpyAsync(base + L.at_members, w.members.data(), w.members.size() * sizeof(TableTextMember), hipMemcpyHostToDevice, cs));
    TRY(hipEventRecord(ev.e[1], cs));
    return MIDAS_SNPS_OK;
  };
  ST_TRY(upload(0, err256));
  std::vector<unsigned long long> bad((size_t)n_tables, ~0ull);
  for (size_t gi = 0; gi < groups.size(); ++gi) {
    const GroupWork& w = work[gi];
    uint8_t* base = static_cast<uint8_t*>(slot[gi & 1].p);
    const SlotLayout L(w.text, w.comp, w.members.size(), w.room, w.cap_lines);
    const size_t nm = w.members.size();
    // (the host's arrays of this group must not change while the copy stream reads them: they are `work`'s, untouched from here on)
    TRY(hipEventSynchronize(ev.e[1]));
    float up = 0.f;
    TRY(hipEventElapsedTime(&up, ev.e[0], ev.e[1]));
    ms[0] += up;
    const InflateParams ip = inflate_params_of(L.infl, base, nm);
    TRY(hipEventRecord(ev.e[2], s));
    TRY(launch_bgzf_inflate(ip, s));
    TRY(hipEventRecord(ev.e[3], s));
    std::vector<uint32_t> status(nm);
    TRY(hipMemcpyAsync(status.data(), ip.status, nm * 4, hipMemcpyDeviceToHost, s));
    // the next group's bytes go up beside these kernels (its slot's last user, group gi - 1, was waited for below)
    if (gi + 1 < groups.size()) ST_TRY(upload(gi + 1, err256));
    TRY(hipStreamSynchronize(s));
    float t_inf = 0.f;
    TRY(hipEventElapsedTime(&t_inf, ev.e[2], ev.e[3]));
    ms[1] += t_inf;
    bool again = false;
    const auto t0 = std::chrono::steady_clock::now();
    ST_TRY(inflate_again(kWho, ip, w.blocks.data(), w.want.data(), status, s, &again, err256));
    if (again) {
      ms[1] += std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
      ++again_total;
    }
    for (size_t k = 0; k < nm; ++k) {
      if (status[k] != 0u) {
        const ChosenMember& c = chosen[groups[gi].lo + k];
        if (err256) snprintf(err256, 256, status[k] == kInflateCrc ? "%s: CRC-32 mismatch in gzip member %d (the inflated bytes are not the ones that were compressed)"
                                                                   : "%s: corrupt deflate data in gzip member %d (code %u)", tableset_path(ts, c.table), c.member, status[k]);
        (void)hipStreamSynchronize(cs);      // (the next group's upload reads host memory of this call)
        return MIDAS_SNPS_ERR_BAD_LAYOUT;
      }
    }
    const TablesScanParams sp = scan_params(L, base, w, tables->d, static_cast<unsigned long long*>(d_bad.p));
    TRY(hipEventRecord(ev.e[2], s));
    TRY(launch_tables_index(sp, s));
    TRY(hipEventRecord(ev.e[3], s));
    TRY(launch_tables_parse(sp, s));
    TRY(hipEventRecord(ev.e[4], s));
    std::vector<uint32_t> lines(nm);
    TRY(hipMemcpyAsync(lines.data(), sp.member_lines, nm * 4, hipMemcpyDeviceToHost, s));
    TRY(hipMemcpyAsync(bad.data(), d_bad.p, (size_t)n_tables * 8, hipMemcpyDeviceToHost, s));
    TRY(hipStreamSynchronize(s));
    float t_idx = 0.f, t_par = 0.f;
    TRY(hipEventElapsedTime(&t_idx, ev.e[2], ev.e[3]));
    TRY(hipEventElapsedTime(&t_par, ev.e[3], ev.e[4]));
    ms[2] += t_idx; ms[3] += t_par;
    comp_total += (int64_t)w.comp; text_total += (int64_t)w.text;
    int32_t st = MIDAS_SNPS_OK;
    for (size_t k = 0; k < nm && st == MIDAS_SNPS_OK; ++k) {
      const TableTextMember& tm = w.members[k];
      if (lines[k] != tm.rows + (tm.header ? 1u : 0u)) {
        if (err256) snprintf(err256, 256, "%s: gzip member %d holds %lld rows and announces %u", tableset_path(ts, (int32_t)tm.table), chosen[groups[gi].lo + k].member,
                             (long long)lines[k] - (tm.header ? 1 : 0), tm.rows);
        st = MIDAS_SNPS_ERR_BAD_LAYOUT;
      }
    }
    for (int32_t t = 0; t < n_tables && st == MIDAS_SNPS_OK; ++t) {
      if (bad[(size_t)t] != ~0ull) {
        if (err256) snprintf(err256, 256, "%s: malformed row %lld", tableset_path(ts, t), (long long)bad[(size_t)t] + 1);
        st = MIDAS_SNPS_ERR_BAD_LAYOUT;
      }
    }
    if (st != MIDAS_SNPS_OK) { (void)hipStreamSynchronize(cs); return st; }
  }
  if (out_stats8) { out_stats8[2] = (int64_t)groups.size(); out_stats8[3] = comp_total; out_stats8[4] = text_total; out_stats8[6] = again_total; }
  if (out_ms4) memcpy(out_ms4, ms, sizeof ms);
  return MIDAS_SNPS_OK;
}

int32_t midas_snps_parse_rows_device(midas_snps_ctx* ctx, const uint8_t* text, int64_t n_bytes, int32_t skip_header, uint32_t* out_counts, int64_t cap_rows,
                                     int64_t* out_rows, int64_t* out_bad_row) {
  if (!ctx || n_bytes < 0 || n_bytes >= ((int64_t)1 << 31) || (n_bytes > 0 && !text) || cap_rows < 0 || (cap_rows > 0 && !out_counts) || !out_rows || !out_bad_row)
    return MIDAS_SNPS_ERR_INVALID_ARG;
  *out_rows = 0;
  *out_bad_row = -1;
  if (n_bytes == 0) return MIDAS_SNPS_OK;
  std::lock_guard<std::mutex> g(ctx->device_mutex);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  GroupWork w;
  w.text = (size_t)n_bytes;
  for (int64_t k = 0; k < n_bytes; ++k) w.cap_lines += text[k] == '\n';      // (sizes the index; what the lines ARE is the kernels' business)
  w.cap_lines += 1;
  TableTextMember tm{};
  tm.start = 0; tm.ulen = (uint32_t)n_bytes; tm.header = skip_header ? 1u : 0u;
  w.members.push_back(tm);
  const SlotLayout L(w.text, 0, 1, 0, w.cap_lines);
  DeviceBuf slot, d_counts, d_bad;
  HIP_TRY(ctx, hipMalloc(&slot.p, L.end));
  HIP_TRY(ctx, hipMalloc(&d_counts.p, std::max<size_t>((size_t)cap_rows * 16, 16)));
  HIP_TRY(ctx, hipMalloc(&d_bad.p, 8));
  uint8_t* base = static_cast<uint8_t*>(slot.p);
  HIP_TRY(ctx, hipMemcpyAsync(base, text, (size_t)n_bytes, hipMemcpyHostToDevice, s));
  HIP_TRY(ctx, hipMemsetAsync(d_bad.p, 0xFF, 8, s));
  HIP_TRY(ctx, hipMemcpyAsync(base + L.at_members, w.members.data(), sizeof(TableTextMember), hipMemcpyHostToDevice, s));
  TablesScanParams sp = scan_params(L, base, w, static_cast<uint32_t*>(d_counts.p), static_cast<unsigned long long*>(d_bad.p));
  HIP_TRY(ctx, launch_tables_index(sp, s));
  uint32_t lines = 0;
  HIP_TRY(ctx, hipMemcpyAsync(&lines, sp.member_lines, 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(ctx, hipStreamSynchronize(s));
  const uint32_t head = skip_header ? 1u : 0u;
  const int64_t rows = lines > head ? (int64_t)(lines - head) : 0;
  *out_rows = rows;
  if (rows == 0) return MIDAS_SNPS_OK;
  if (lines > w.cap_lines) return fail(ctx, MIDAS_SNPS_ERR_HIP, "row parser: more lines indexed than the text has line ends");
  // the rows are known now: the member announces them, the first cap_rows are taken
  w.members[0].rows = (uint32_t)rows;
  w.members[0].take = (uint32_t)std::min(rows, cap_rows);
  w.n_take = (long long)w.members[0].take;
  HIP_TRY(ctx, hipMemcpyAsync(base + L.at_members, w.members.data(), sizeof(TableTextMember), hipMemcpyHostToDevice, s));
  sp.n_take = w.n_take;
  HIP_TRY(ctx, launch_tables_parse(sp, s));
  unsigned long long bad = ~0ull;
  HIP_TRY(ctx, hipMemcpyAsync(&bad, d_bad.p, 8, hipMemcpyDeviceToHost, s));
  if (w.n_take > 0) HIP_TRY(ctx, hipMemcpyAsync(out_counts, d_counts.p, (size_t)w.n_take * 16, hipMemcpyDeviceToHost, s));
  HIP_TRY(ctx, hipStreamSynchronize(s));
  if (bad != ~0ull) *out_bad_row = (int64_t)bad;
  return MIDAS_SNPS_OK;
}

}  // extern "C"
