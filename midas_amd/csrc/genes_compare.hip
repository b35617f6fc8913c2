// compare_genes.py on MI355X: the distance of the gene content of every pair of samples, from genes_copynum.txt as text.
//
//   open     the matrix is mapped; its header gives the sample ids, its newlines the row count (host)
//   chunks   a run of bytes is uploaded; its complete rows are the group's candidates        (text_rows.h, as sites_rows.h)
//   index    newlines counted per 16 bytes, exclusive scan, newline k's position -> ends[k]   (text_rows.h)
//   parse    one thread a row walks its fields; the cells of the first S sample columns are converted as pandas' C reader
//            converts them (genes_rows.h, pandas_f64.h: NOT float()), sample-major [sample][G].  A row of another width or a cell that is
//            no finite decimal literal is reported by (row, column), the earliest in file order
//   bits     --dtype presabs: one wave a (sample, 64 genes): value > cutoff, the ballot is a word of the bit matrix; the pair
//            counts are ss_pairs_kernel's popcounts (text_rows.h), integers held on the device across groups
//   ordered  --dtype copynum: sum of min(a, b), of max(a, b) and of (a - b)^2 or |a - b| over the genes IN ROW ORDER, as
//   pairs    Python's sum() over np.float64 forms them: one fp64 add per gene, left to right, from 0.  A workgroup owns a
//            64 x 64 tile of pairs and the whole gene axis of the group; a thread keeps a 4 x 4 patch of pairs in registers.
//            The gene axis is never split or tree-reduced: the order of additions is the result.  Across row groups the sums
//            live in [S][S] device arrays, loaded at a group's start and stored at its end, so the bits cannot depend on
//            group_rows or chunk_bytes
//   write    the pair table, numbers as str() writes them (host)
// Compiled with -ffp-contract=off (build.py): (a - b) * (a - b) and the add after it round separately.
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <charconv>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <string_view>
#include <vector>

#include "../../include/midas_snps.h"
#include "ctx_internal.h"
#include "genes_rows.h"
#include "kernels.h"
#include "pandas_f64.h"
#include "text_rows.h"

namespace midas {
namespace {

constexpr int kGeneRun = 32;        // genes of every sample of a strip staged at a time: 2 x 32 x 65 doubles = 33 KB of LDS

// presabs: bits[s][w] bit k = val[s][64 w + k] > cutoff
__global__ __launch_bounds__(256) void gc_bits_kernel(const double* val, long long g, long long stride, int S, double cutoff,
                                                      unsigned long long* bits, long long wstride) {
  const int s = blockIdx.y * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (s >= S) return;                                  // (the whole wave)
  const long long k = (long long)blockIdx.x * 64 + lane;
  const bool present = k < g && val[(long long)s * stride + k] > cutoff;
  const unsigned long long word = __ballot(present);
  if (lane == 0) bits[(long long)s * wstride + blockIdx.x] = word;
}

// copynum: for i <= j, over the group's genes in order: both[i][j] += min(a, b), either[i][j] += max(a, b) and (kDist 1)
// dist[i][j] += (a - b) * (a - b) or (kDist 2) += |a - b|, a = val[i][k], b = val[j][k]; min / max with Python's tie rule.
// Tiles, staging and the 4 x 4 patches as ss_pairs_kernel; blockIdx.x counts the tiles on or above the diagonal.  No other
// workgroup touches this tile's sums and the genes are walked front to back: every sum is the sequential one, bit for bit.
template <int kDist>
__global__ __launch_bounds__(256) void gc_ordered_pairs_kernel(const double* val, long long stride, long long g, int S, int tiles_side,
                                                               double* both, double* either, double* dist) {
  __shared__ double sa[kGeneRun][kPairPad], sb[kGeneRun][kPairPad];
  int ti = 0, left = blockIdx.x;
  while (left >= tiles_side - ti) { left -= tiles_side - ti; ++ti; }
  const int tj = ti + left;
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  double xb[4][4], xe[4][4], xd[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int gi = ti * kPairTile + ty + 16 * i, gj = tj * kPairTile + tx + 16 * j;
      const bool mine = gi <= gj && gj < S;
      const long long at = (long long)gi * S + gj;
      xb[i][j] = mine ? both[at] : 0.0;
      xe[i][j] = mine ? either[at] : 0.0;
      xd[i][j] = (kDist != 0 && mine) ? dist[at] : 0.0;
    }
  for (long long k0 = 0; k0 < g; k0 += kGeneRun) {
#pragma unroll
    for (int it = 0; it < kPairTile * kGeneRun / 256; ++it) {
      const int e = it * 256 + tid, s = e / kGeneRun, k = e % kGeneRun;
      const long long w = k0 + k;
      const int gi = ti * kPairTile + s, gj = tj * kPairTile + s;
      sa[k][s] = (gi < S && w < g) ? val[(long long)gi * stride + w] : 0.0;
      sb[k][s] = (gj < S && w < g) ? val[(long long)gj * stride + w] : 0.0;
    }
    __syncthreads();
    const int kn = g - k0 < kGeneRun ? (int)(g - k0) : kGeneRun;
    for (int k = 0; k < kn; ++k) {
      double a[4], b[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) { a[i] = sa[k][ty + 16 * i]; b[i] = sb[k][tx + 16 * i]; }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          xb[i][j] += b[j] < a[i] ? b[j] : a[i];
          xe[i][j] += b[j] > a[i] ? b[j] : a[i];
          if (kDist == 1) {
            const double d = a[i] - b[j];
            xd[i][j] += d * d;
          } else if (kDist == 2) {
            xd[i][j] += fabs(a[i] - b[j]);
          }
        }
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int gi = ti * kPairTile + ty + 16 * i, gj = tj * kPairTile + tx + 16 * j;
      if (gi <= gj && gj < S) {
        const long long at = (long long)gi * S + gj;
        both[at] = xb[i][j];
        either[at] = xe[i][j];
        if (kDist != 0) dist[at] = xd[i][j];
      }
    }
}

}  // namespace
}  // namespace midas

using namespace midas;

extern "C" {

int32_t midas_genes_matrix_open(const char* path, midas_genes_matrix** out, char* err1024) {
  if (!path || !out) return MIDAS_SNPS_ERR_INVALID_ARG;
  *out = nullptr;
  if (err1024) err1024[0] = 0;
  midas_genes_matrix* m = new midas_genes_matrix();
  m->path = path;
  const int fd = ::open(path, O_RDONLY);
  struct stat st;
  if (fd < 0 || fstat(fd, &st) != 0) {
    if (fd >= 0) ::close(fd);
    gm_fail(err1024, m->path, 0, "cannot be read");
    delete m;
    return MIDAS_SNPS_ERR_INVALID_ARG;
  }
  m->size = (size_t)st.st_size;
  if (m->size) {
    void* p = mmap(nullptr, m->size, PROT_READ, MAP_PRIVATE, fd, 0);
    if (p == MAP_FAILED) {
      ::close(fd);
      m->size = 0;
      gm_fail(err1024, m->path, 0, "cannot be mapped");
      delete m;
      return MIDAS_SNPS_ERR_INVALID_ARG;
    }
    m->base = static_cast<const char*>(p);
  }
  ::close(fd);
  if (m->size == 0) {
    gm_fail(err1024, m->path, 0, "is empty");
    delete m;
    return MIDAS_SNPS_ERR_BAD_LAYOUT;
  }
  const char* nl = static_cast<const char*>(memchr(m->base, '\n', m->size));
  size_t e = nl ? (size_t)(nl - m->base) : m->size;
  m->body = nl ? e + 1 : m->size;
  if (e > 0 && m->base[e - 1] == '\r') --e;
  size_t p = 0;
  bool first = true;
  for (size_t q = 0;; ++q) {
    if (q == e || m->base[q] == '\t') {
      if (first) m->first_field.assign(m->base + p, q - p);
      else {
        m->id_pool.insert(m->id_pool.end(), m->base + p, m->base + q);
        m->id_off.push_back((int64_t)m->id_pool.size());
      }
      first = false;
      if (q == e) break;
      p = q + 1;
    }
  }
  const char* s = m->base + m->body;
  const size_t n = m->size - m->body;
  int64_t rows = 0;
  for (const char* q = s; q < s + n;) {
    const char* x = static_cast<const char*>(memchr(q, '\n', (size_t)(s + n - q)));
    ++rows;
    if (!x) break;
    q = x + 1;
  }
  m->n_rows = rows;
  *out = m;
  return MIDAS_SNPS_OK;
}

int32_t midas_genes_matrix_counts(const midas_genes_matrix* m, int64_t* out4) {
  if (!m || !out4) return MIDAS_SNPS_ERR_INVALID_ARG;
  out4[0] = (int64_t)m->id_off.size() - 1;
  out4[1] = m->n_rows;
  out4[2] = (int64_t)(m->size - m->body);
  out4[3] = (int64_t)m->id_pool.size();
  return MIDAS_SNPS_OK;
}

int32_t midas_genes_matrix_columns(const midas_genes_matrix* m, const void** out4, int64_t* out_first_bytes) {
  if (!m || !out4 || !out_first_bytes) return MIDAS_SNPS_ERR_INVALID_ARG;
  out4[0] = m->id_pool.data();
  out4[1] = m->id_off.data();
  out4[2] = m->base + m->body;
  out4[3] = m->first_field.data();
  *out_first_bytes = (int64_t)m->first_field.size();
  return MIDAS_SNPS_OK;
}

void midas_genes_matrix_close(midas_genes_matrix* m) { delete m; }

int32_t midas_genes_compare_parse_cell(const char* text, int64_t n, double* out, int32_t* out_plain_int) {
  if (!text || n < 0 || n > 0x7FFFFFFF || !out) return MIDAS_SNPS_ERR_INVALID_ARG;
  bool plain = true;
  if (!pandas_f64(text, (int)n, out, &plain)) return MIDAS_SNPS_ERR_BAD_LAYOUT;
  if (out_plain_int) *out_plain_int = plain ? 1 : 0;
  return MIDAS_SNPS_OK;
}

int32_t midas_genes_compare(midas_snps_ctx* ctx, const char* text, int64_t text_bytes, int64_t n_rows_max, int32_t n_samples,
                            int32_t n_columns, int32_t dtype, int32_t distance, double cutoff, const int64_t* iparams4,
                            int64_t* out_count, double* out_both, double* out_either, double* out_dist, uint8_t* out_col_float,
                            double* dump_cells, int64_t* out_stats16, float* out_ms8) {
  if (!ctx || text_bytes < 0 || (text_bytes > 0 && !text) || n_rows_max < 0 || n_samples < 1 || n_columns < n_samples || !iparams4 ||
      !out_stats16 || iparams4[0] < 0 || iparams4[1] < 0 || (dtype != MIDAS_GENES_PRESABS && dtype != MIDAS_GENES_COPYNUM) ||
      distance < MIDAS_GENES_JACCARD || distance > MIDAS_GENES_MANHATTAN || !out_col_float)
    return MIDAS_SNPS_ERR_INVALID_ARG;
  const bool copynum = dtype == MIDAS_GENES_COPYNUM;
  const int S = n_samples, kdist = copynum ? distance : 0;
  if (copynum ? (!out_both || !out_either || (kdist != 0 && !out_dist)) : !out_count) return MIDAS_SNPS_ERR_INVALID_ARG;
  ctx->clear_error();
  ctx->err_read = -1;
  for (int k = 0; k < 16; ++k) out_stats16[k] = 0;
  out_stats16[5] = -1;
  out_stats16[6] = -1;
  if (out_ms8) for (int k = 0; k < 8; ++k) out_ms8[k] = 0.f;
  const size_t n_acc = (size_t)S * (size_t)S;
  for (size_t k = 0; k < n_acc; ++k) {
    if (!copynum) out_count[k] = 0;
    else { out_both[k] = 0.0; out_either[k] = 0.0; if (kdist) out_dist[k] = 0.0; }
  }
  for (int s = 0; s < S; ++s) out_col_float[s] = 0;
  if (n_rows_max == 0 || text_bytes == 0) return MIDAS_SNPS_OK;
  SS_TRY(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  SsBufs dev;
  SsEvents ev;
  float ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};     // upload + index (host clock), index, parse, bit matrix, pairs, -, -, download
  // ---- sizes: rows a group and bytes a chunk, from the caller or from a quarter of the free device memory --------------------
  constexpr long long kChunkMax = 1ll << 30;    // newline offsets are 32-bit
  long long G = iparams4[0], chunk_bytes = iparams4[1];
  const long long per_row = (long long)S * 8 + (S + 7) / 8 + 4;
  if (G == 0 || chunk_bytes == 0) {
    size_t free_b = 0, total_b = 0;
    SS_TRY(hipMemGetInfo(&free_b, &total_b));
    const long long budget = (long long)(free_b / 4);
    if (chunk_bytes == 0) chunk_bytes = std::min<long long>(kChunkMax, std::max<long long>(1 << 20, budget / 4));
    if (G == 0) G = std::max<long long>(1, (budget - std::min(budget / 2, 5 * chunk_bytes / 4)) / per_row);
  }
  chunk_bytes = std::min(std::max<long long>(chunk_bytes, 64), kChunkMax);
  chunk_bytes = std::min(chunk_bytes, std::max<long long>(64, (long long)text_bytes + 1));
  G = std::max<long long>(1, std::min<long long>(std::min<long long>(G, n_rows_max), chunk_bytes));
  const size_t cells = (size_t)G * (size_t)S;
  if (cells > 0xFFFFFFF0ull) return ss_fail(ctx, MIDAS_SNPS_ERR_UNSUPPORTED, "a row group beyond 2^32 cells: lower group_rows");
  for (auto& x : ev.e) SS_TRY(hipEventCreate(&x));
  Chunk ck;
  ck.host = text;
  ck.bytes = text_bytes;
  {
    const int32_t rc = chunk_alloc(ctx, dev, ck, chunk_bytes);
    if (rc != MIDAS_SNPS_OK) return rc;
  }
  const long long wstride = (G + 63) / 64;
  uint32_t *d_scratch = nullptr, *d_col_float = nullptr;
  double *d_val = nullptr, *d_both = nullptr, *d_either = nullptr, *d_dist = nullptr;
  unsigned long long *d_bits = nullptr, *d_count = nullptr;
  SS_TRY(dev.get(&ck.d_ends, ((size_t)G + 1) * 4));
  SS_TRY(dev.get(&ck.d_bad, 8));
  SS_TRY(dev.get(&d_scratch, scan_scratch_words((kChunkMax + 16) / 16) * 4));
  SS_TRY(dev.get(&d_val, cells * 8));
  SS_TRY(dev.get(&d_col_float, (size_t)S * 4));
  SS_TRY(hipMemsetAsync(d_col_float, 0, (size_t)S * 4, st));
  if (copynum) {
    SS_TRY(dev.get(&d_both, n_acc * 8));
    SS_TRY(dev.get(&d_either, n_acc * 8));
    SS_TRY(hipMemsetAsync(d_both, 0, n_acc * 8, st));
    SS_TRY(hipMemsetAsync(d_either, 0, n_acc * 8, st));
    if (kdist) {
      SS_TRY(dev.get(&d_dist, n_acc * 8));
      SS_TRY(hipMemsetAsync(d_dist, 0, n_acc * 8, st));
    }
  } else {
    SS_TRY(dev.get(&d_bits, (size_t)S * (size_t)wstride * 8));
    SS_TRY(dev.get(&d_count, n_acc * 8));
    SS_TRY(hipMemsetAsync(d_count, 0, n_acc * 8, st));
  }
  const int tiles_side = (S + kPairTile - 1) / kPairTile;
  const long long n_tiles = (long long)tiles_side * (tiles_side + 1) / 2;
  const long long pair_blocks = iparams4[2] > 0 ? iparams4[2] : 1024;      // presabs: workgroups the popcount kernel aims at
  long long base = 0, groups = 0, steps = 0;
  while (base < n_rows_max) {
    const auto t_load = std::chrono::steady_clock::now();
    {
      const int32_t rc = chunk_load(ctx, st, ev, ck, chunk_bytes, G, d_scratch, &ms[1]);
      if (rc != MIDAS_SNPS_OK) return rc;
    }
    ms[0] += std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_load).count();
    const long long g = std::min(ck.lines, std::min(G, n_rows_max - base));
    if (g == 0) {
      if (ck.at_eof) break;
      if (chunk_bytes >= kChunkMax) return ss_fail(ctx, MIDAS_SNPS_ERR_UNSUPPORTED, "a matrix row longer than 1 GiB");
      chunk_bytes = std::min(kChunkMax, chunk_bytes * 2);
      const int32_t rc = chunk_alloc(ctx, dev, ck, chunk_bytes);
      if (rc != MIDAS_SNPS_OK) return rc;
      continue;
    }
    ++groups;
    // ---- parse -------------------------------------------------------------------------------------------------------------
    SS_TRY(hipMemsetAsync(ck.d_bad, 0xFF, 8, st));
    SS_TRY(hipEventRecord(ev.e[2], st));
    GcParseP pp;
    pp.text = ck.d_text; pp.ends = ck.d_ends; pp.g = g; pp.stride = G; pp.S = S; pp.n_cols = n_columns; pp.val = d_val;
    pp.col_float = d_col_float; pp.bad = ck.d_bad;
    hipLaunchKernelGGL(gc_parse_kernel, dim3(nblocks(g, 256)), dim3(256), 0, st, pp);
    SS_TRY(hipGetLastError());
    SS_TRY(hipEventRecord(ev.e[3], st));
    // ---- pairs -------------------------------------------------------------------------------------------------------------
    if (copynum) {
      if (kdist == 0) hipLaunchKernelGGL(gc_ordered_pairs_kernel<0>, dim3((unsigned)n_tiles), dim3(256), 0, st, d_val, G, g, S, tiles_side, d_both, d_either, d_dist);
      else if (kdist == 1) hipLaunchKernelGGL(gc_ordered_pairs_kernel<1>, dim3((unsigned)n_tiles), dim3(256), 0, st, d_val, G, g, S, tiles_side, d_both, d_either, d_dist);
      else hipLaunchKernelGGL(gc_ordered_pairs_kernel<2>, dim3((unsigned)n_tiles), dim3(256), 0, st, d_val, G, g, S, tiles_side, d_both, d_either, d_dist);
      SS_TRY(hipGetLastError());
      SS_TRY(hipEventRecord(ev.e[4], st));
      SS_TRY(hipEventRecord(ev.e[5], st));
      steps += (long long)S * (S + 1) / 2 * g;
    } else {
      const long long n_words = (g + 63) / 64;
      hipLaunchKernelGGL(gc_bits_kernel, dim3((unsigned)n_words, (unsigned)((S + 3) / 4)), dim3(256), 0, st, d_val, g, G, S, cutoff, d_bits, wstride);
      SS_TRY(hipGetLastError());
      SS_TRY(hipEventRecord(ev.e[4], st));
      const PairRuns pr = pair_runs(n_words, n_tiles, pair_blocks, kPairRun);
      hipLaunchKernelGGL(ss_pairs_kernel, dim3((unsigned)n_tiles, (unsigned)pr.runs), dim3(256), 0, st, d_bits, wstride, n_words, pr.run_words,
                         S, tiles_side, d_count);
      SS_TRY(hipGetLastError());
      SS_TRY(hipEventRecord(ev.e[5], st));
      steps += (long long)S * (S + 1) / 2 * n_words;
    }
    unsigned long long bad = kNoBad;
    uint32_t end_at = 0;
    SS_TRY(hipMemcpyAsync(&bad, ck.d_bad, 8, hipMemcpyDeviceToHost, st));
    SS_TRY(hipMemcpyAsync(&end_at, ck.d_ends + g - 1, 4, hipMemcpyDeviceToHost, st));
    if (dump_cells)
      for (int s = 0; s < S; ++s)
        SS_TRY(hipMemcpyAsync(dump_cells + (size_t)s * (size_t)n_rows_max + base, d_val + (size_t)s * G, (size_t)g * 8, hipMemcpyDeviceToHost, st));
    SS_TRY(hipStreamSynchronize(st));
    float t = 0.f;
    SS_TRY(hipEventElapsedTime(&t, ev.e[2], ev.e[3]));
    ms[2] += t;
    SS_TRY(hipEventElapsedTime(&t, ev.e[3], ev.e[4]));
    ms[copynum ? 4 : 3] += t;
    SS_TRY(hipEventElapsedTime(&t, ev.e[4], ev.e[5]));
    if (!copynum) ms[4] += t;
    if (bad != kNoBad) {          // the groups come in file order and a group reports its earliest: the file's earliest
      const long long row = base + (long long)(bad >> 32), col = (long long)(bad & 0xFFFFFFFFull) - 1;
      out_stats16[0] = base;
      out_stats16[4] = col < 0 ? 1 : 2;
      out_stats16[5] = row;
      out_stats16[6] = col;
      char buf[160];
      if (col < 0) snprintf(buf, sizeof buf, "data row %lld: not %d sample columns wide", row, n_columns);
      else snprintf(buf, sizeof buf, "data row %lld, sample column %lld: not a finite decimal number", row, col);
      return ss_fail(ctx, MIDAS_SNPS_ERR_BAD_LAYOUT, buf);
    }
    base += g;
    ck.at = std::min(ck.bytes, ck.at + (long long)end_at + 1);
  }
  std::vector<uint32_t> col_float((size_t)S, 0u);
  SS_TRY(hipEventRecord(ev.e[0], st));
  SS_TRY(hipMemcpyAsync(col_float.data(), d_col_float, (size_t)S * 4, hipMemcpyDeviceToHost, st));
  if (copynum) {
    SS_TRY(hipMemcpyAsync(out_both, d_both, n_acc * 8, hipMemcpyDeviceToHost, st));
    SS_TRY(hipMemcpyAsync(out_either, d_either, n_acc * 8, hipMemcpyDeviceToHost, st));
    if (kdist) SS_TRY(hipMemcpyAsync(out_dist, d_dist, n_acc * 8, hipMemcpyDeviceToHost, st));
  } else {
    SS_TRY(hipMemcpyAsync(out_count, d_count, n_acc * 8, hipMemcpyDeviceToHost, st));
  }
  SS_TRY(hipEventRecord(ev.e[1], st));
  SS_TRY(hipStreamSynchronize(st));
  float t = 0.f;
  SS_TRY(hipEventElapsedTime(&t, ev.e[0], ev.e[1]));
  ms[7] += t;
  for (int s = 0; s < S; ++s) out_col_float[s] = col_float[(size_t)s] ? 1 : 0;
  out_stats16[0] = base;
  out_stats16[7] = groups;
  out_stats16[8] = steps;
  out_stats16[9] = G;
  out_stats16[10] = chunk_bytes;
  out_stats16[11] = n_tiles;
  if (out_ms8) for (int k = 0; k < 8; ++k) out_ms8[k] = ms[k];
  return MIDAS_SNPS_OK;
}

// sample1, sample2, count1, count2, count_both, count_either, distance for every pair i < j of the first n_samples columns
int32_t midas_genes_compare_write_pairs(const char* path, const midas_genes_matrix* m, int32_t n_samples, int32_t dtype, int32_t distance,
                                        int64_t n_rows, const int64_t* count, const double* both, const double* either, const double* dist,
                                        char* err1024) {
  if (!path || !m || n_samples < 1 || n_samples > (int64_t)m->id_off.size() - 1 || n_rows < 0 ||
      (dtype != MIDAS_GENES_PRESABS && dtype != MIDAS_GENES_COPYNUM) || distance < MIDAS_GENES_JACCARD || distance > MIDAS_GENES_MANHATTAN)
    return MIDAS_SNPS_ERR_INVALID_ARG;
  const bool copynum = dtype == MIDAS_GENES_COPYNUM;
  if (copynum ? (!both || !either || (distance != MIDAS_GENES_JACCARD && !dist)) : !count) return MIDAS_SNPS_ERR_INVALID_ARG;
  if (err1024) err1024[0] = 0;
  FILE* f = fopen(path, "w");
  if (!f) { gm_fail(err1024, path, 0, "cannot be written"); return MIDAS_SNPS_ERR_INVALID_ARG; }
  std::string buf;
  buf.reserve(1 << 20);
  bool ok = true;
  auto put_f64 = [&](double v) {
    char tmp[40];
    int64_t n = 0;
    midas_genes_merge_format_f64(1, &v, tmp, sizeof tmp, &n);
    buf.append(tmp, (size_t)(n > 0 ? n - 1 : 0));      // (without the formatter's '\n')
  };
  auto put_i64 = [&](int64_t v) {
    char tmp[24];
    buf.append(tmp, (size_t)(std::to_chars(tmp, tmp + sizeof tmp, v).ptr - tmp));
  };
  auto id = [&](int64_t s) { return std::string_view(m->id_pool.data() + m->id_off[(size_t)s], (size_t)(m->id_off[(size_t)s + 1] - m->id_off[(size_t)s])); };
  buf += "sample1\tsample2\tcount1\tcount2\tcount_both\tcount_either\tdistance\n";
  const int64_t S = n_samples;
  for (int64_t i = 0; i < S; ++i)
    for (int64_t j = i + 1; j < S; ++j) {
      buf.append(id(i));
      buf.push_back('\t');
      buf.append(id(j));
      buf.push_back('\t');
      if (!copynum) {
        const int64_t c1 = count[i * S + i], c2 = count[j * S + j], b = count[i * S + j], u = c1 + c2 - b, diff = c1 + c2 - 2 * b;
        const int64_t v[4] = {c1, c2, b, u};
        for (int c = 0; c < 4; ++c) { put_i64(v[c]); buf.push_back('\t'); }
        if (distance == MIDAS_GENES_JACCARD) {
          if (u > 0) put_f64(1.0 - (double)b / (double)u); else buf.push_back('0');
        } else if (distance == MIDAS_GENES_EUCLIDEAN) {
          put_f64(std::sqrt((double)diff));
        } else {
          put_f64((double)diff);
        }
      } else if (n_rows == 0) {
        // no row was read: every sum() is the integer it started from
        buf += "0\t0\t0\t0\t";
        if (distance == MIDAS_GENES_JACCARD) buf.push_back('0'); else buf += "0.0";
      } else {
        // count1 and count2 are both the second sample's sum, as the reference writes them; min(a, a) = a gives it
        const double c2 = both[j * S + j], b = both[i * S + j], u = either[i * S + j];
        const double v[4] = {c2, c2, b, u};
        for (int c = 0; c < 4; ++c) { put_f64(v[c]); buf.push_back('\t'); }
        if (distance == MIDAS_GENES_JACCARD) {
          if (u > 0) put_f64(1.0 - b / u); else buf.push_back('0');
        } else if (distance == MIDAS_GENES_EUCLIDEAN) {
          put_f64(std::sqrt(dist[i * S + j]));
        } else {
          put_f64(dist[i * S + j]);
        }
      }
      buf.push_back('\n');
      if (buf.size() > (1u << 20) - 4096) {
        ok = fwrite(buf.data(), 1, buf.size(), f) == buf.size() && ok;
        buf.clear();
      }
    }
  ok = (buf.empty() || fwrite(buf.data(), 1, buf.size(), f) == buf.size()) && ok;
  ok = fclose(f) == 0 && ok;
  if (!ok) { gm_fail(err1024, path, 0, "cannot be written"); return MIDAS_SNPS_ERR_INVALID_ARG; }
  return MIDAS_SNPS_OK;
}

}  // extern "C"
