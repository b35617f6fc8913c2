// compare_genes.py on MI355X: the distance of the gene content of every pair of samples, from genes_copynum.txt as text.
//
//   open     the matrix is mapped; its header gives the sample ids, its newlines the row count (host)
//   rows     the walk by row groups is GeneRows' (genes_rows.h), shared with genes_linkage.hip:
//     chunks a run of bytes is uploaded; its complete rows are the group's candidates        (text_rows.h, as sites_rows.h)
//     index  newlines counted per 16 bytes, exclusive scan, newline k's position -> ends[k]   (text_rows.h)
//     parse  one thread a row walks its fields; the cells of the first S sample columns are converted as pandas' C reader
//            converts them (pandas_f64.h: NOT float()), sample-major [sample][G].  A row of another width or a cell that is
//            no finite decimal literal is reported by (row, column), the earliest in file order
//   bits     --dtype presabs: one wave a (sample, 64 genes): value > cutoff, the ballot is a word of the bit matrix
//            (planes_by_sample_kernel over PresentCell, bit_planes.h); the pair counts are ss_pairs_kernel's popcounts
//            (text_rows.h), integers held on the device across groups
//   ordered  --dtype copynum: sum of min(a, b), of max(a, b) and of (a - b)^2 or |a - b| over the genes IN ROW ORDER, as
//   pairs    Python's sum() over np.float64 forms them: one fp64 add per gene, left to right, from 0.  A workgroup owns a
//            64 x 64 tile of pairs and the whole gene axis of the group; a thread keeps a 4 x 4 patch of pairs in registers.
//            The gene axis is never split or tree-reduced: the order of additions is the result.  Across row groups the sums
//            live in [S][S] device arrays, loaded at a group's start and stored at its end, so the bits cannot depend on
//            group_rows or chunk_bytes
//   write    the pair table, numbers as str() writes them (host; TableWriter, genes_rows.h)
// Compiled with -ffp-contract=off (build.py): (a - b) * (a - b) and the add after it round separately.
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
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

// copynum: for i <= j, over the group's genes in order: both[i][j] += min(a, b), either[i][j] += max(a, b) and (kDist 1)
// dist[i][j] += (a - b) * (a - b) or (kDist 2) += |a - b|, a = val[i][k], b = val[j][k]; min / max with Python's tie rule.
// Tiles, staging and the 4 x 4 patches as ss_pairs_kernel; blockIdx.x counts the tiles on or above the diagonal.  No other
// workgroup touches this tile's sums and the genes are walked front to back: every sum is the sequential one, bit for bit.
template <int kDist>
__global__ __launch_bounds__(256) void gc_ordered_pairs_kernel(const double* val, long long stride, long long g, int S, int tiles_side,
                                                               double* both, double* either, double* dist) {
  __shared__ double sa[kGeneRun][kPairPad], sb[kGeneRun][kPairPad];
  const PairTile tile = pair_tile(blockIdx.x, tiles_side);
  const int ti = tile.ti, tj = tile.tj;
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
  if ((dtype != MIDAS_GENES_PRESABS && dtype != MIDAS_GENES_COPYNUM) || distance < MIDAS_GENES_JACCARD || distance > MIDAS_GENES_MANHATTAN ||
      !out_col_float)
    return MIDAS_SNPS_ERR_INVALID_ARG;
  const bool copynum = dtype == MIDAS_GENES_COPYNUM;
  const int S = n_samples, kdist = copynum ? distance : 0;
  if (copynum ? (!out_both || !out_either || (kdist != 0 && !out_dist)) : !out_count) return MIDAS_SNPS_ERR_INVALID_ARG;
  {
    const int32_t rc = genes_begin(ctx, text, text_bytes, n_rows_max, S, n_columns, iparams4, out_stats16, out_ms8);
    if (rc != MIDAS_SNPS_OK) return rc;
  }
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
  GeneRows rows(ctx, dev, ev, ms, out_stats16);
  {
    const int32_t rc = rows.init(text, text_bytes, n_rows_max, S, n_columns, iparams4[0], iparams4[1], (long long)S * 8 + (S + 7) / 8 + 4, 0);
    if (rc != MIDAS_SNPS_OK) return rc;
  }
  const long long G = rows.G, wstride = (G + 63) / 64;
  double *d_val = rows.d_val, *d_both = nullptr, *d_either = nullptr, *d_dist = nullptr;
  unsigned long long *d_bits = nullptr, *d_count = nullptr;
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
  const PairTiles tiles = pair_tiles(S, kPairTile);
  const long long pair_blocks = iparams4[2] > 0 ? iparams4[2] : 1024;      // presabs: workgroups the popcount kernel aims at
  long long steps = 0;
  for (;;) {
    long long g = 0;
    {
      const int32_t rc = rows.next(&g);
      if (rc != MIDAS_SNPS_OK) return rc;
    }
    if (g == 0) break;
    // ---- pairs, queued behind the parse: a group with a bad row adds to sums nobody downloads -------------------------------------
    if (copynum) {
      if (kdist == 0) hipLaunchKernelGGL(gc_ordered_pairs_kernel<0>, dim3((unsigned)tiles.n), dim3(256), 0, st, d_val, G, g, S, tiles.side, d_both, d_either, d_dist);
      else if (kdist == 1) hipLaunchKernelGGL(gc_ordered_pairs_kernel<1>, dim3((unsigned)tiles.n), dim3(256), 0, st, d_val, G, g, S, tiles.side, d_both, d_either, d_dist);
      else hipLaunchKernelGGL(gc_ordered_pairs_kernel<2>, dim3((unsigned)tiles.n), dim3(256), 0, st, d_val, G, g, S, tiles.side, d_both, d_either, d_dist);
      SS_TRY(hipGetLastError());
      SS_TRY(hipEventRecord(ev.e[4], st));
      steps += (long long)S * (S + 1) / 2 * g;
    } else {
      const long long n_words = (g + 63) / 64;
      hipLaunchKernelGGL((planes_by_sample_kernel<1, PresentCell>), dim3((unsigned)n_words, (unsigned)((S + 3) / 4)), dim3(256), 0, st,
                         PresentCell{d_val, G, cutoff}, g, S, wstride, d_bits, (unsigned long long*)nullptr);
      SS_TRY(hipGetLastError());
      SS_TRY(hipEventRecord(ev.e[4], st));
      const PairRuns pr = pair_runs(n_words, tiles.n, pair_blocks, kPairRun);
      hipLaunchKernelGGL(ss_pairs_kernel, dim3((unsigned)tiles.n, (unsigned)pr.runs), dim3(256), 0, st, d_bits, wstride, n_words, pr.run_words,
                         S, tiles.side, d_count);
      SS_TRY(hipGetLastError());
      SS_TRY(hipEventRecord(ev.e[5], st));
      steps += (long long)S * (S + 1) / 2 * n_words;
    }
    if (dump_cells)
      for (int s = 0; s < S; ++s)
        SS_TRY(hipMemcpyAsync(dump_cells + (size_t)s * (size_t)n_rows_max + rows.base, d_val + (size_t)s * G, (size_t)g * 8, hipMemcpyDeviceToHost, st));
    {
      const int32_t rc = rows.check(g);
      if (rc != MIDAS_SNPS_OK) return rc;
    }
    SS_TRY(rows.lap(3, 4, copynum ? 4 : 3));
    if (!copynum) SS_TRY(rows.lap(4, 5, 4));
    rows.advance(g);
  }
  std::vector<uint32_t> col_float((size_t)S, 0u);
  SS_TRY(hipEventRecord(ev.e[0], st));
  SS_TRY(hipMemcpyAsync(col_float.data(), rows.d_col_float, (size_t)S * 4, hipMemcpyDeviceToHost, st));
  if (copynum) {
    SS_TRY(hipMemcpyAsync(out_both, d_both, n_acc * 8, hipMemcpyDeviceToHost, st));
    SS_TRY(hipMemcpyAsync(out_either, d_either, n_acc * 8, hipMemcpyDeviceToHost, st));
    if (kdist) SS_TRY(hipMemcpyAsync(out_dist, d_dist, n_acc * 8, hipMemcpyDeviceToHost, st));
  } else {
    SS_TRY(hipMemcpyAsync(out_count, d_count, n_acc * 8, hipMemcpyDeviceToHost, st));
  }
  SS_TRY(hipEventRecord(ev.e[1], st));
  SS_TRY(hipStreamSynchronize(st));
  SS_TRY(rows.lap(0, 1, 7));
  for (int s = 0; s < S; ++s) out_col_float[s] = col_float[(size_t)s] ? 1 : 0;
  out_stats16[8] = steps;
  out_stats16[11] = tiles.n;
  rows.end(out_ms8);
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
  TableWriter w(path);
  if (!w.f) { gm_fail(err1024, path, 0, "cannot be written"); return MIDAS_SNPS_ERR_INVALID_ARG; }
  std::string& buf = w.buf;
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
        for (int c = 0; c < 4; ++c) { w.i64(v[c]); buf.push_back('\t'); }
        if (distance == MIDAS_GENES_JACCARD) {
          if (u > 0) w.f64(1.0 - (double)b / (double)u); else buf.push_back('0');
        } else if (distance == MIDAS_GENES_EUCLIDEAN) {
          w.f64(std::sqrt((double)diff));
        } else {
          w.f64((double)diff);
        }
      } else if (n_rows == 0) {
        // no row was read: every sum() is the integer it started from
        buf += "0\t0\t0\t0\t";
        if (distance == MIDAS_GENES_JACCARD) buf.push_back('0'); else buf += "0.0";
      } else {
        // count1 and count2 are both the second sample's sum, as the reference writes them; min(a, a) = a gives it
        const double c2 = both[j * S + j], b = both[i * S + j], u = either[i * S + j];
        const double v[4] = {c2, c2, b, u};
        for (int c = 0; c < 4; ++c) { w.f64(v[c]); buf.push_back('\t'); }
        if (distance == MIDAS_GENES_JACCARD) {
          if (u > 0) w.f64(1.0 - b / u); else buf.push_back('0');
        } else if (distance == MIDAS_GENES_EUCLIDEAN) {
          w.f64(std::sqrt(dist[i * S + j]));
        } else {
          w.f64(dist[i * S + j]);
        }
      }
      w.row_done();
    }
  if (!w.close()) { gm_fail(err1024, path, 0, "cannot be written"); return MIDAS_SNPS_ERR_INVALID_ARG; }
  return MIDAS_SNPS_OK;
}

}  // extern "C"
