// `merge_midas.py snps` on MI355X: the rows of snps_freq.txt / snps_depth.txt formatted on the device, from the per-sample
// depth / minor-count arrays where merge_sites.hip leaves them ([sample][site] u32), into the very bytes
// midas_merge_write_matrix (tables_host.cpp) writes: `site_id \t v[0] \t ... \t v[S-1] \n` per kept site, v = str(depth) or
// '{0:.3g}'.format(float(minor) / depth if depth > 0 else 0.0) (merge_fmt.h: integers, no printf).
//
//   compact   flag byte of the calls word == 0 -> scan -> the kept sites of the chunk, in order
//   length    one thread per kept row: the bytes of the row; scanned (launch_scan_u32) into where the rows start
//   write     a wave takes 64 consecutive kept rows, lane = row: the loads of a sample's row are 64 neighbouring sites.  The
//             samples are walked eight at a time (any number of samples: a whole row need not fit anywhere); a lane formats
//             its eight cells into its slot of LDS, then the wave moves the slots out one row at a time, lane = byte: every
//             store instruction writes one contiguous run of the file, not 64 scattered bytes.
// The scan is 32-bit, so the rows go in batches whose text stays below a cap (MIDAS_SNPS_MERGE_TEXT_MB, default 256; a
// single row longer than the cap is a batch by itself); where a batch starts in the file is the host's 64-bit business.
#include <hip/hip_runtime.h>

#include <fcntl.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/midas_snps.h"
#include "ctx_internal.h"
#include "kernels.h"
#include "merge_fmt.h"
#include "merge_rows.h"

namespace midas {
namespace {

constexpr int kRowsPerWave = 64;     // rows of a workgroup (one wave)
constexpr int kGroup = 8;            // samples formatted between two moves out of LDS
// a lane's slot: the site id (<= 19 digits), eight cells of a tab and <= 10 digits, the newline = 108 bytes; 33 words, so that
// the lanes' slots start in different banks
constexpr int kSlot = 132;
constexpr long long kIdBytes = 20;   // site id + newline
constexpr long long kDepthCell = 11, kFreqCell = 9;     // tab + digits

struct RowsKParams {
  const uint32_t* depth;       // [n_samples][m]
  const uint32_t* minor;       // [n_samples][m], or nullptr: the depth table
  const uint32_t* keep;        // the batch's kept rows: indices < m
  uint32_t* len;               // [n_rows + 1]
  uint8_t* text;
  unsigned long long* err;     // lowest row of the batch with minor > depth > 0, else ~0
  long long id_base;
  uint32_t m, n_rows;
  int n_samples;
};

__global__ __launch_bounds__(256) void rows_keep_flag_kernel(const uint32_t* calls, uint32_t m, uint32_t* flag) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < m) flag[i] = (calls[i] >> 24) == 0u ? 1u : 0u;
  if (i == m) flag[i] = 0u;
}

__global__ __launch_bounds__(256) void rows_keep_scatter_kernel(const uint32_t* calls, uint32_t m, const uint32_t* rank, uint32_t* keep) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < m && (calls[i] >> 24) == 0u) keep[rank[i]] = i;
}

__global__ __launch_bounds__(256) void rows_length_kernel(RowsKParams p) {
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  if (r > p.n_rows) return;
  if (r == p.n_rows) { p.len[r] = 0u; return; }               // the scan leaves the batch's total here
  const uint32_t i = p.keep[r];
  uint32_t n = midas_fmt::digits_u64((uint64_t)(p.id_base + (long long)i + 1)) + (uint32_t)p.n_samples + 1u;
  bool bad = false;
#pragma unroll 4
  for (int s = 0; s < p.n_samples; ++s) {
    const size_t at = (size_t)s * p.m + i;
    const uint32_t d = p.depth[at];
    if (p.minor) {
      const uint32_t mc = p.minor[at];
      if (mc > d && d > 0u) { bad = true; n += 1u; }
      else n += midas_fmt::freq_cell(mc, d).len;
    } else {
      n += midas_fmt::digits_u32(d);
    }
  }
  p.len[r] = n;
  if (bad) atomicMin(p.err, (unsigned long long)r);
}

__global__ __launch_bounds__(kRowsPerWave) void rows_write_kernel(RowsKParams p) {
  __shared__ uint8_t s_seg[kRowsPerWave * kSlot];
  __shared__ uint32_t s_at[kRowsPerWave], s_n[kRowsPerWave];
  const int lane = threadIdx.x;
  const uint32_t r = blockIdx.x * (uint32_t)kRowsPerWave + (uint32_t)lane;
  const bool live = r < p.n_rows;
  const uint32_t i = live ? p.keep[r] : 0u;
  uint32_t at = live ? p.len[r] : 0u;                          // where the row starts in the batch's text
  uint8_t* const slot = s_seg + lane * kSlot;
  for (int s0 = 0; s0 < p.n_samples; s0 += kGroup) {
    uint32_t dv[kGroup], mv[kGroup];
#pragma unroll
    for (int g = 0; g < kGroup; ++g) {                         // the group's loads first: eight in flight per lane
      const bool ok = live && s0 + g < p.n_samples;
      const size_t a = ok ? (size_t)(s0 + g) * p.m + i : 0;
      dv[g] = ok ? p.depth[a] : 0u;
      mv[g] = ok && p.minor ? p.minor[a] : 0u;
    }
    uint32_t n = 0;
    if (live) {
      if (s0 == 0) {
        const uint64_t id = (uint64_t)(p.id_base + (long long)i + 1);
        const uint32_t nd = midas_fmt::digits_u64(id);
        midas_fmt::put_decimal(slot, id, nd);
        n = nd;
      }
#pragma unroll
      for (int g = 0; g < kGroup; ++g) {
        if (s0 + g < p.n_samples) {
          slot[n++] = '\t';
          if (p.minor) {
            // (a minor count above its depth never gets here: the length pass refuses the batch)
            const midas_fmt::Cell c = midas_fmt::freq_cell(mv[g] <= dv[g] ? mv[g] : 0u, dv[g]);
            for (uint32_t b = 0; b < c.len; ++b) slot[n + b] = (uint8_t)(c.bytes >> (8u * b));
            n += c.len;
          } else {
            const uint32_t nd = midas_fmt::digits_u32(dv[g]);
            midas_fmt::put_decimal32(slot + n, dv[g], nd);
            n += nd;
          }
        }
      }
      if (s0 + kGroup >= p.n_samples) slot[n++] = '\n';
    }
    s_at[lane] = at;
    s_n[lane] = n;
    at += n;
    __syncthreads();
    for (int j = 0; j < kRowsPerWave; ++j) {                   // row j's run of the file, lane = byte
      const uint32_t nj = s_n[j], aj = s_at[j];
      for (uint32_t b = (uint32_t)lane; b < nj; b += (uint32_t)kRowsPerWave) p.text[(size_t)aj + b] = s_seg[j * kSlot + b];
    }
    __syncthreads();
  }
}

int32_t rfail(midas_snps_ctx* ctx, int32_t st, const char* what, hipError_t e) {
  char buf[384];
  snprintf(buf, sizeof buf, "%s: %s", what, hipGetErrorString(e));
  (void)hipGetLastError();
  ctx->set_error(buf);
  return st;
}

#define R_TRY(call)                                                                                                 \
  do {                                                                                                              \
    hipError_t e__ = (call);                                                                                        \
    if (e__ != hipSuccess) return rfail(ctx_, e__ == hipErrorOutOfMemory ? MIDAS_SNPS_ERR_OUT_OF_MEMORY : MIDAS_SNPS_ERR_HIP, #call, e__); \
  } while (0)

double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// the cap on a batch's text, bytes: MIDAS_SNPS_MERGE_TEXT_MB (a fraction is allowed: 0.004 is 4 KiB), 1 KiB .. 1 GiB
size_t text_cap() {
  double mb = 256.0;
  if (const char* e = getenv("MIDAS_SNPS_MERGE_TEXT_MB")) {
    const double v = atof(e);
    if (v > 0.0) mb = v;
  }
  double bytes = mb * 1048576.0;
  if (bytes < 1024.0) bytes = 1024.0;
  if (bytes > 1073741824.0) bytes = 1073741824.0;
  return (size_t)bytes;
}

}  // namespace

// ---- the file ---------------------------------------------------------------------------------------------------------------
namespace {
bool pwrite_all(int fd, const uint8_t* p, size_t n, long long off) {
  while (n > 0) {
    const ssize_t w = pwrite(fd, p, n, (off_t)off);
    if (w <= 0) return false;
    p += w; n -= (size_t)w; off += w;
  }
  return true;
}
}  // namespace

bool MergeTextFile::open(const char* final_path, const char* header_line) {
  path = final_path;
  tmp = path + ".tmp." + std::to_string((long long)getpid());
  fd = ::open(tmp.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0666);
  if (fd < 0) return false;
  const size_t n = strlen(header_line);
  off = (long long)n;
  return pwrite_all(fd, reinterpret_cast<const uint8_t*>(header_line), n, 0);
}
bool MergeTextFile::commit() {
  if (fd < 0) return false;
  const bool closed = ::close(fd) == 0;
  fd = -1;
  if (!closed || rename(tmp.c_str(), path.c_str()) != 0) { (void)remove(tmp.c_str()); tmp.clear(); return false; }
  tmp.clear();
  return true;
}
MergeTextFile::~MergeTextFile() {
  if (fd >= 0) (void)::close(fd);
  if (!tmp.empty()) (void)remove(tmp.c_str());
}

// ---- the ring's file side ---------------------------------------------------------------------------------------------------
MergeTextSink::MergeTextSink(midas_snps_ctx* ctx) : ctx_(ctx) {}

int32_t MergeTextSink::start() {
  ctx_->stage_join();
  for (int k = 0; k < midas_snps_ctx::kStageSlots; ++k)
    if (!ctx_->stage[k]) R_TRY(hipHostMalloc(&ctx_->stage[k], midas_snps_ctx::kStageBytes, midas_ctx::kHostAllocFlags));
  thread_ = std::thread([this] { run(); });
  started_ = true;
  return MIDAS_SNPS_OK;
}

void MergeTextSink::run() {
  for (;;) {
    Slot job;
    bool skip;
    int k;
    {
      std::unique_lock<std::mutex> g(m_);
      k = (int)(written_ % midas_snps_ctx::kStageSlots);        // the slots are filled in turn, and written in that order
      cv_.wait(g, [&] { return stop_ || slot_[k].full; });
      if (!slot_[k].full) return;
      job = slot_[k];
      skip = failed_;                                            // (after a failure the slots are only emptied)
    }
    const double t0 = now_s();
    const bool ok = skip || pwrite_all(job.to->fd, static_cast<const uint8_t*>(ctx_->stage[k]), job.n, job.off);
    {
      std::lock_guard<std::mutex> g(m_);
      write_s += now_s() - t0;
      if (!ok) failed_ = true;
      slot_[k].full = false;
      ++written_;
    }
    cv_.notify_all();
  }
}

int32_t MergeTextSink::send(MergeTextFile* to, const uint8_t* d_text, size_t n) {
  constexpr size_t kChunk = midas_snps_ctx::kStageBytes;
  for (size_t off = 0; off < n; off += kChunk) {
    const size_t len = std::min(kChunk, n - off);
    const int k = (int)(sent_ % midas_snps_ctx::kStageSlots);
    {
      std::unique_lock<std::mutex> g(m_);
      cv_.wait(g, [&] { return !slot_[k].full; });
      if (failed_) { ctx_->set_error("write failed on " + to->path); return MIDAS_SNPS_ERR_INVALID_ARG; }
    }
    const double t0 = now_s();
    const int32_t st = midas_ctx::copy_to_host(ctx_, ctx_->stage[k], d_text + off, len);      // (page-locked target: no ring inside)
    if (st != MIDAS_SNPS_OK) return st;
    copy_s += now_s() - t0;
    bytes += (long long)len;
    {
      std::lock_guard<std::mutex> g(m_);
      slot_[k].to = to;
      slot_[k].n = len;
      slot_[k].off = to->off;
      to->off += (long long)len;
      slot_[k].full = true;
      ++sent_;
    }
    cv_.notify_all();
  }
  return MIDAS_SNPS_OK;
}

bool MergeTextSink::finish() {
  if (started_) {
    {
      std::unique_lock<std::mutex> g(m_);
      cv_.wait(g, [&] { return written_ == sent_; });
      stop_ = true;
    }
    cv_.notify_all();
    thread_.join();
    started_ = false;
  }
  return !failed_;
}

MergeTextSink::~MergeTextSink() { (void)finish(); }

// ---- the formatter ----------------------------------------------------------------------------------------------------------
MergeRowFormatter::~MergeRowFormatter() {
  for (void* q : {(void*)d_len_, (void*)d_rank_, (void*)d_keep_, (void*)d_scratch_, (void*)d_text_, (void*)d_err_})
    if (q) (void)hipFree(q);
  if (h_down_) (void)hipHostFree(h_down_);
  if (e0_) (void)hipEventDestroy(e0_);
  if (e1_) (void)hipEventDestroy(e1_);
}

int32_t MergeRowFormatter::prepare(long long max_rows, bool with_compact) {
  if (max_rows < 1) max_rows = 1;
  max_rows_ = max_rows;
  const long long row_max = kIdBytes + kDepthCell * (long long)n_samples_;
  if (row_max >= (1ll << 31)) { ctx_->set_error("merge rows: too many samples for one row"); return MIDAS_SNPS_ERR_UNSUPPORTED; }
  text_cap_ = text_cap();
  // the text buffer: the cap, or one row where a row is longer -- and no more than the call's rows can fill
  long long need = std::max<long long>((long long)text_cap_, row_max);
  if (max_rows < need / row_max + 1) need = std::max(row_max, max_rows * row_max);
  text_bytes_ = ((size_t)need + 15) & ~(size_t)15;
  R_TRY(hipMalloc(&d_len_, ((size_t)max_rows + 1) * 4));
  if (with_compact) {
    R_TRY(hipMalloc(&d_rank_, ((size_t)max_rows + 1) * 4));
    R_TRY(hipMalloc(&d_keep_, (size_t)max_rows * 4));
  }
  R_TRY(hipMalloc(&d_scratch_, (scan_scratch_words(max_rows + 1) + 16) * 4));
  R_TRY(hipMalloc(&d_text_, text_bytes_));
  R_TRY(hipMalloc(&d_err_, 8));
  R_TRY(hipHostMalloc(reinterpret_cast<void**>(&h_down_), 16, midas_ctx::kHostAllocFlags));
  h_down_[0] = h_down_[1] = 0ull;
  R_TRY(hipEventCreate(&e0_));
  R_TRY(hipEventCreate(&e1_));
  return MIDAS_SNPS_OK;
}

int32_t MergeRowFormatter::compact(const uint32_t* d_calls, uint32_t m, const uint32_t** d_keep, long long* n_keep) {
  *d_keep = d_keep_;
  *n_keep = 0;
  if (m == 0u) return MIDAS_SNPS_OK;
  if ((long long)m > max_rows_ || !d_rank_) { ctx_->set_error("merge rows: chunk larger than prepared"); return MIDAS_SNPS_ERR_INVALID_ARG; }
  hipStream_t st = ctx_->stream;
  const unsigned grid = (unsigned)(((unsigned long long)m + 1 + 255) / 256);
  R_TRY(hipEventRecord(e0_, st));
  hipLaunchKernelGGL(rows_keep_flag_kernel, dim3(grid), dim3(256), 0, st, d_calls, m, d_rank_);
  R_TRY(hipGetLastError());
  R_TRY(launch_scan_u32(d_rank_, d_rank_, (long long)m + 1, d_scratch_, st));
  hipLaunchKernelGGL(rows_keep_scatter_kernel, dim3(grid), dim3(256), 0, st, d_calls, m, d_rank_, d_keep_);
  R_TRY(hipGetLastError());
  R_TRY(hipEventRecord(e1_, st));
  uint32_t kept = 0;
  R_TRY(hipMemcpyAsync(&kept, d_rank_ + m, 4, hipMemcpyDeviceToHost, st));
  R_TRY(hipStreamSynchronize(st));
  float ms = 0.f;
  R_TRY(hipEventElapsedTime(&ms, e0_, e1_));
  format_ms += ms;
  *n_keep = (long long)kept;
  return MIDAS_SNPS_OK;
}

int32_t MergeRowFormatter::emit(const uint32_t* d_depth, const uint32_t* d_minor, uint32_t m, const uint32_t* d_keep, long long n_keep,
                                long long id_base, MergeTextSink* sink, MergeTextFile* to) {
  if (n_keep <= 0) return MIDAS_SNPS_OK;
  hipStream_t st = ctx_->stream;
  const long long row_max = kIdBytes + (d_minor ? kFreqCell : kDepthCell) * (long long)n_samples_;
  long long batch_rows = (long long)text_cap_ / row_max;
  if (batch_rows < 1) batch_rows = 1;
  if (batch_rows > max_rows_) batch_rows = max_rows_;
  if (batch_rows * row_max > (long long)text_bytes_) batch_rows = std::max<long long>(1, (long long)text_bytes_ / row_max);
  for (long long r0 = 0; r0 < n_keep; r0 += batch_rows) {
    const long long nr = std::min(batch_rows, n_keep - r0);
    RowsKParams p;
    p.depth = d_depth; p.minor = d_minor; p.keep = d_keep + r0; p.len = d_len_; p.text = d_text_; p.err = d_err_;
    p.id_base = id_base; p.m = m; p.n_rows = (uint32_t)nr; p.n_samples = n_samples_;
    R_TRY(hipMemsetAsync(d_err_, 0xFF, 8, st));
    R_TRY(hipEventRecord(e0_, st));
    hipLaunchKernelGGL(rows_length_kernel, dim3((unsigned)((nr + 1 + 255) / 256)), dim3(256), 0, st, p);
    R_TRY(hipGetLastError());
    R_TRY(launch_scan_u32(d_len_, d_len_, nr + 1, d_scratch_, st));
    R_TRY(hipMemcpyAsync(&h_down_[0], d_len_ + nr, 4, hipMemcpyDeviceToHost, st));
    R_TRY(hipMemcpyAsync(&h_down_[1], d_err_, 8, hipMemcpyDeviceToHost, st));
    R_TRY(hipStreamSynchronize(st));
    const uint32_t total = (uint32_t)h_down_[0];
    const unsigned long long err = h_down_[1];
    if (err != ~0ull) {
      ctx_->set_error("merge rows: a minor count above its depth (kept row " + std::to_string(r0 + (long long)err) + ")");
      return MIDAS_SNPS_ERR_INVALID_ARG;
    }
    if ((size_t)total > text_bytes_) {                          // (cannot happen: row_max bounds every row)
      ctx_->set_error("merge rows: a batch's text outgrew its buffer");
      return MIDAS_SNPS_ERR_BAD_LAYOUT;
    }
    hipLaunchKernelGGL(rows_write_kernel, dim3((unsigned)((nr + kRowsPerWave - 1) / kRowsPerWave)), dim3(kRowsPerWave), 0, st, p);
    R_TRY(hipGetLastError());
    R_TRY(hipEventRecord(e1_, st));
    const int32_t sst = sink->send(to, d_text_, (size_t)total);      // (same stream: behind the kernel, and waited for)
    if (sst != MIDAS_SNPS_OK) return sst;
    float ms = 0.f;
    R_TRY(hipEventElapsedTime(&ms, e0_, e1_));
    format_ms += ms;
  }
  return MIDAS_SNPS_OK;
}

}  // namespace midas

// ---- the drop-in writer: host arrays up, rows formatted on the device, text down ------------------------------------------------
namespace {
int32_t wfail(midas_snps_ctx* ctx, int32_t st, const std::string& msg) { ctx->set_error(msg); return st; }
}  // namespace

#define W_TRY(call)                                                                                             \
  do {                                                                                                          \
    hipError_t e__ = (call);                                                                                    \
    if (e__ != hipSuccess) {                                                                                    \
      for (void* q__ : dev) (void)hipFree(q__);                                                                 \
      return midas::rfail(ctx, e__ == hipErrorOutOfMemory ? MIDAS_SNPS_ERR_OUT_OF_MEMORY : MIDAS_SNPS_ERR_HIP, #call, e__); \
    }                                                                                                           \
  } while (0)

extern "C" int32_t midas_merge_write_matrix_device(midas_snps_ctx* ctx, const char* path, const char* header_line, int64_t n_keep,
                                                   const int64_t* keep, int32_t n_samples, int64_t n_sites, const uint32_t* depth,
                                                   const uint32_t* minor_count, int64_t site_id_base, float* out_format_ms) {
  if (!ctx || !path || !header_line || n_keep < 0 || n_samples <= 0 || n_sites < 0 || site_id_base < 0 || (n_keep > 0 && (!keep || !depth)))
    return MIDAS_SNPS_ERR_INVALID_ARG;
  ctx->clear_error();
  if (out_format_ms) *out_format_ms = 0.f;
  // the device reads depth[s * m + keep]: every kept row must be a site of the arrays
  bool ascending = true;
  for (int64_t r = 0; r < n_keep; ++r) {
    if (keep[r] < 0 || keep[r] >= n_sites) return wfail(ctx, MIDAS_SNPS_ERR_INVALID_ARG, "merge_write_matrix_device: keep[" + std::to_string(r) + "] is no site of the arrays");
    if (r > 0 && keep[r] < keep[r - 1]) ascending = false;
  }
  // the arrays go up in chunks of sites, as the merge kernel's tables do: <= ~2 GiB of the two arrays at a time
  long long chunk = (long long)((2ull << 30) / (8ull * (unsigned long long)n_samples));
  if (chunk < 1024) chunk = 1024;
  if (chunk > (1ll << 26)) chunk = 1ll << 26;
  if (const char* e = getenv("MIDAS_SNPS_MERGE_CHUNK_SITES")) {      // developer knob: chunk borders with small inputs
    const long long v = atoll(e);
    if (v > 0 && v < chunk) chunk = v;
  }
  if (chunk > n_sites) chunk = n_sites > 0 ? n_sites : 1;
  if (!ascending && n_sites > chunk)
    return wfail(ctx, MIDAS_SNPS_ERR_UNSUPPORTED, "merge_write_matrix_device: kept rows out of order in arrays larger than one chunk");
  std::lock_guard<std::mutex> ring(ctx->copy_mutex);
  std::vector<void*> dev;
  W_TRY(hipSetDevice(ctx->device));
  midas::MergeTextFile file;
  if (!file.open(path, header_line)) return wfail(ctx, MIDAS_SNPS_ERR_INVALID_ARG, std::string("cannot open ") + path + " for writing");
  midas::MergeTextSink sink(ctx);
  midas::MergeRowFormatter fmt(ctx, n_samples);
  int32_t st = MIDAS_SNPS_OK;
  if (n_keep > 0) {
    if ((st = sink.start()) != MIDAS_SNPS_OK) return st;
    long long keep_cap = n_keep;                                // the most kept rows a chunk holds (a site may be kept twice)
    if (ascending && n_sites > chunk) {
      keep_cap = 1;
      for (int64_t a = 0, b = 0; a < n_keep; a = b) {
        const long long end = (keep[a] / chunk + 1) * chunk;
        while (b < n_keep && keep[b] < end) ++b;
        keep_cap = std::max<long long>(keep_cap, b - a);
      }
    }
    if ((st = fmt.prepare(keep_cap, false)) != MIDAS_SNPS_OK) return st;
    uint32_t* d_depth = nullptr; uint32_t* d_minor = nullptr; uint32_t* d_keep = nullptr;
    W_TRY(hipMalloc(&d_depth, (size_t)chunk * n_samples * 4)); dev.push_back(d_depth);
    if (minor_count) { W_TRY(hipMalloc(&d_minor, (size_t)chunk * n_samples * 4)); dev.push_back(d_minor); }
    W_TRY(hipMalloc(&d_keep, (size_t)keep_cap * 4)); dev.push_back(d_keep);
    std::vector<uint32_t> local((size_t)keep_cap);
    int64_t r = 0;
    for (long long lo = 0; lo < n_sites && r < n_keep && st == MIDAS_SNPS_OK; lo += chunk) {
      const long long m = std::min(chunk, (long long)n_sites - lo);
      int64_t r1 = r;
      if (ascending) { while (r1 < n_keep && keep[r1] < lo + m) ++r1; } else { r1 = n_keep; }
      if (r1 == r) continue;
      for (int64_t k = r; k < r1; ++k) local[(size_t)(k - r)] = (uint32_t)(keep[k] - lo);
      for (int s = 0; s < n_samples; ++s) {
        W_TRY(hipMemcpyAsync(d_depth + (size_t)s * m, depth + (size_t)s * n_sites + lo, (size_t)m * 4, hipMemcpyHostToDevice, ctx->stream));
        if (minor_count)
          W_TRY(hipMemcpyAsync(d_minor + (size_t)s * m, minor_count + (size_t)s * n_sites + lo, (size_t)m * 4, hipMemcpyHostToDevice, ctx->stream));
      }
      W_TRY(hipMemcpyAsync(d_keep, local.data(), (size_t)(r1 - r) * 4, hipMemcpyHostToDevice, ctx->stream));
      W_TRY(hipStreamSynchronize(ctx->stream));
      st = fmt.emit(d_depth, d_minor, (uint32_t)m, d_keep, r1 - r, (long long)site_id_base + lo, &sink, &file);
      r = r1;
    }
  }
  const bool written = sink.finish();
  for (void* q : dev) (void)hipFree(q);
  if (st != MIDAS_SNPS_OK) return st;
  if (!written || !file.commit()) return wfail(ctx, MIDAS_SNPS_ERR_INVALID_ARG, std::string("write failed on ") + path);
  if (out_format_ms) *out_format_ms = fmt.format_ms;
  if (getenv("MIDAS_SNPS_TRACE"))
    fprintf(stderr, "[merge rows] %s: format %.3f ms (device), text down %.3f s, file write %.3f s on the writer thread, %lld bytes of text\n",
            minor_count ? "freq" : "depth", fmt.format_ms, sink.copy_s, sink.write_s, sink.bytes);
  return MIDAS_SNPS_OK;
}
