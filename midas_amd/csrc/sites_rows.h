// The rows of snps_freq.txt / snps_depth.txt on the device, for every entry point that walks the two matrices: sites_scan.hip
// (snp_diversity.py, call_consensus.py), sites_strains.hip (strain_tracking.py) and sites_trees.hip (snp_trees.py).  The matrices
// arrive as TEXT; parsing them is most of the work, so it happens here.
//
//   chunks   a run of bytes of each matrix is uploaded; its complete rows are the group's candidates
//   index    newlines counted per 16 bytes, the library's exclusive scan (device_sort.hip), newline k's position -> ends[k]
//   parse    one thread a row walks its fields; a cell of a selected sample is converted on the spot when it has the shape
//            [+-]digits[.digits][e[+-]digits] with a mantissa below 2^53 and a power of ten within +-22 (one exact
//            int -> fp64 conversion, one IEEE multiply or divide: correctly rounded), or [+-]digits up to 18 of them for
//            the depth; every other cell goes to a side list, which the host converts with its exact parser and patches
//            in before the caller's kernels run.  Values land sample-major, [sample][row]
// (chunks, the line index, the pair tiles and the popcount pair kernel live in text_rows.h, shared with genes_rows.h; the sizes of
// a walk are row_group_plan.h's, the kernels that turn calls into bit planes bit_planes.h's)
// Also here: what the entry points check and set up alike before the walk (sites_begin), and the statistics they all close
// with (sites_end).  Everything has internal linkage: each of the files compiles its own copy, with -ffp-contract=off
// (build.py): fast_f64's one multiply or divide must stay one.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <string>
#include <string_view>
#include <vector>

#include "../../include/midas_snps.h"
#include "ctx_internal.h"
#include "kernels.h"
#include "row_group_plan.h"
#include "text_numbers.h"
#include "text_rows.h"

namespace midas {
namespace {

// float(cell) for [+-]digits[.digits][e[+-]digits], mantissa < 2^53, |power of ten| <= 22: exact by construction
__device__ bool fast_f64(const char* s, int n, double* out) {
  static const double p10[23] = {1e0,  1e1,  1e2,  1e3,  1e4,  1e5,  1e6,  1e7,  1e8,  1e9,  1e10, 1e11,
                                 1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};
  if (n <= 0) return false;
  int i = 0;
  bool neg = false;
  if (s[0] == '+' || s[0] == '-') { neg = s[0] == '-'; i = 1; }
  unsigned long long m = 0;
  constexpr unsigned long long lim = (1ull << 53) - 1;
  int nd = 0, nfrac = 0;
  for (; i < n && is_digit(s[i]); ++i, ++nd) {
    const unsigned d = (unsigned)(s[i] - '0');
    if (m > (lim - d) / 10) return false;
    m = m * 10 + d;
  }
  if (nd == 0) return false;
  if (i < n && s[i] == '.') {
    for (++i; i < n && is_digit(s[i]); ++i, ++nfrac) {
      const unsigned d = (unsigned)(s[i] - '0');
      if (m > (lim - d) / 10) return false;
      m = m * 10 + d;
    }
    if (nfrac == 0) return false;
  }
  int ex = 0;
  if (i < n && (s[i] == 'e' || s[i] == 'E')) {
    ++i;
    bool eneg = false;
    if (i < n && (s[i] == '+' || s[i] == '-')) { eneg = s[i] == '-'; ++i; }
    int ne = 0;
    for (; i < n && is_digit(s[i]); ++i, ++ne) {
      if (ne == 3) return false;
      ex = ex * 10 + (s[i] - '0');
    }
    if (ne == 0) return false;
    if (eneg) ex = -ex;
  }
  if (i != n) return false;
  double x = (double)(long long)m;
  if (m != 0) {
    const int e10 = ex - nfrac;
    if (e10 < -22 || e10 > 22) return false;
    x = e10 < 0 ? __ddiv_rn(x, p10[-e10]) : __dmul_rn(x, p10[e10]);
  }
  *out = neg ? -x : x;
  return true;
}

// int(cell) for [+-]digits, at most 18 digits
__device__ bool fast_i64(const char* s, int n, long long* out) {
  if (n <= 0) return false;
  int i = 0;
  bool neg = false;
  if (s[0] == '+' || s[0] == '-') { neg = s[0] == '-'; i = 1; }
  if (i == n || n - i > 18) return false;
  long long m = 0;
  for (; i < n; ++i) {
    if (!is_digit(s[i])) return false;
    m = m * 10 + (s[i] - '0');
  }
  *out = neg ? -m : m;
  return true;
}

struct ParseP {
  const char* text;            // the chunk
  const uint32_t* ends;        // newline offsets of its rows
  long long g, stride;         // rows to parse; row stride of a sample's values
  const int32_t* col_slot;     // [n_cols] matrix column -> selected sample, or -1
  int n_cols;                  // columns a row must have (1 + the largest selected column)
  void* val;                   // [n_samples][stride] f64 or i64
  SideCell* side;
  uint32_t* side_n;
  uint32_t side_cap;
  unsigned long long* bad;     // min over (row << 32 | slot + 1); slot + 1 == 0: the row is short
};

template <bool kInt>
__global__ __launch_bounds__(256) void ss_parse_kernel(ParseP p) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r >= p.g) return;
  const uint32_t b = r == 0 ? 0u : p.ends[r - 1] + 1u;
  uint32_t e = p.ends[r];
  const char* t = p.text;
  if (e > b && t[e - 1] == '\r') --e;
  uint32_t q = b;
  while (q < e && t[q] != '\t') ++q;         // the site id
  for (int c = 0; c < p.n_cols; ++c) {
    if (q >= e) {                            // no tab left: the row lacks column c
      atomicMin(p.bad, (unsigned long long)r << 32);
      return;
    }
    const uint32_t fs = ++q;
    while (q < e && t[q] != '\t') ++q;
    const int slot = p.col_slot[c];
    if (slot < 0) continue;
    const int len = (int)(q - fs);
    const long long at = (long long)slot * p.stride + r;
    bool ok;
    if (kInt) {
      long long v = 0;
      ok = fast_i64(t + fs, len, &v);
      static_cast<long long*>(p.val)[at] = v;
    } else {
      double v = 0.0;
      ok = fast_f64(t + fs, len, &v);
      static_cast<double*>(p.val)[at] = v;
    }
    if (!ok) {
      const uint32_t k = atomicAdd(p.side_n, 1u);
      if (k < p.side_cap) p.side[k] = SideCell{(uint32_t)r, (uint32_t)slot, fs, (uint32_t)len};
    }
  }
}

template <class T>
__global__ __launch_bounds__(256) void ss_patch_kernel(T* val, const long long* at, const T* v, long long n) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) val[at[i]] = v[i];
}

// What every entry point over the two matrices checks and sets up alike, after the checks that are its own: the matrices, the
// row and sample counts and the statistics array are there, every sample selects a column; then the context's error and the
// caller's statistics and times are reset, and col_slot maps a matrix column to the sample that selected it -- no column twice.
int32_t sites_begin(midas_snps_ctx* ctx, const char* freq, int64_t freq_bytes, const char* depth, int64_t depth_bytes, int64_t n_rows,
                    int32_t n_samples, const int32_t* sample_col, int64_t* out_stats16, float* out_ms8, std::vector<int32_t>* col_slot) {
  if (!ctx || freq_bytes < 0 || depth_bytes < 0 || (freq_bytes > 0 && !freq) || (depth_bytes > 0 && !depth) || n_rows < 0 ||
      n_samples < 1 || !sample_col || !out_stats16)
    return MIDAS_SNPS_ERR_INVALID_ARG;
  int n_cols = 0;
  for (int s = 0; s < n_samples; ++s) {
    if (sample_col[s] < 0) return MIDAS_SNPS_ERR_INVALID_ARG;
    n_cols = std::max(n_cols, sample_col[s] + 1);
  }
  ctx->clear_error();
  ctx->err_read = -1;
  for (int k = 0; k < 16; ++k) out_stats16[k] = 0;
  out_stats16[5] = -1;
  out_stats16[6] = -1;
  if (out_ms8) for (int k = 0; k < 8; ++k) out_ms8[k] = 0.f;
  col_slot->assign((size_t)n_cols, -1);
  for (int s = 0; s < n_samples; ++s) {
    if ((*col_slot)[(size_t)sample_col[s]] >= 0) return ss_fail(ctx, MIDAS_SNPS_ERR_INVALID_ARG, "a matrix column is selected twice");
    (*col_slot)[(size_t)sample_col[s]] = s;
  }
  return MIDAS_SNPS_OK;
}

// The rows of the two matrices on the device, a group at a time: upload, line index, cell parse, side-list patching.  Every
// entry point walks the tables through it: next() leaves the group's cells in d_fv / d_dv, [sample][G].
struct RowGroups {
  midas_snps_ctx* ctx;
  hipStream_t st;
  SsBufs& dev;
  SsEvents& ev;                  // e[1], e[2], e[3] are used here
  float* ms;                     // [0] upload + index (host clock), [1] index, [2] parse
  int64_t* stats;                // the caller's out_stats16: [2] / [3] cells converted by the host, [0], [4..6] on a bad row
  int S = 0, n_cols = 0;
  long long G = 0, chunk_bytes = 0, n_sites_max = 0;
  size_t cells = 0;
  Chunk ck[2];
  uint32_t* d_scratch = nullptr;
  double* d_fv = nullptr;
  long long* d_dv = nullptr;
  int32_t* d_col_slot = nullptr;
  long long* d_patch_at = nullptr;
  void* d_patch_v = nullptr;
  size_t patch_cap = 0;
  std::vector<SideCell> side_h;
  std::vector<long long> patch_at;
  std::vector<double> patch_f;
  std::vector<long long> patch_i;
  long long base = 0, groups = 0;
  uint32_t end_at[2] = {0, 0};
  unsigned long long bad[2] = {kNoBad, kNoBad};

  RowGroups(midas_snps_ctx* c, SsBufs& d, SsEvents& e, float* ms8, int64_t* stats16) : ctx(c), st(c->stream), dev(d), ev(e), ms(ms8), stats(stats16) {}

  int32_t alloc_chunk(Chunk& c, long long cb) { return chunk_alloc(ctx, dev, c, cb); }

  // sizes: rows a group (G) and bytes a chunk, from the caller or from a quarter of the free device memory; per_row = the
  // device bytes a row of the group takes in the caller's and in these buffers
  int32_t init(const char* freq, long long freq_bytes, const char* depth, long long depth_bytes, long long n_max, int n_samples,
               const std::vector<int32_t>& col_slot, long long G_in, long long chunk_in, long long per_row) {
    S = n_samples;
    n_cols = (int)col_slot.size();
    n_sites_max = n_max;
    size_t free_b = 0, total_b = 0;
    if (G_in == 0 || chunk_in == 0) SS_TRY(hipMemGetInfo(&free_b, &total_b));
    const RowGroupPlan plan = plan_row_groups(free_b, G_in, chunk_in, 2, std::max(freq_bytes, depth_bytes), n_sites_max, per_row);
    G = plan.G;
    chunk_bytes = plan.chunk_bytes;
    cells = (size_t)G * (size_t)S;
    if (cells > 0xFFFFFFF0ull) return ss_fail(ctx, MIDAS_SNPS_ERR_UNSUPPORTED, "a row group beyond 2^32 cells: lower group_rows");
    for (auto& x : ev.e) SS_TRY(hipEventCreate(&x));
    ck[0].host = freq; ck[0].bytes = freq_bytes;
    ck[1].host = depth; ck[1].bytes = depth_bytes;
    for (Chunk& c : ck) {
      int32_t rc = alloc_chunk(c, chunk_bytes);
      if (rc != MIDAS_SNPS_OK) return rc;
      SS_TRY(dev.get(&c.d_ends, ((size_t)G + 1) * 4));
      SS_TRY(dev.get(&c.d_side, cells * sizeof(SideCell)));
      SS_TRY(dev.get(&c.d_side_n, 4));
      SS_TRY(dev.get(&c.d_bad, 8));
    }
    SS_TRY(dev.get(&d_scratch, std::max(scan_scratch_words((kChunkMax + 16) / 16), scan_scratch_words(G)) * 4));
    SS_TRY(dev.get(&d_fv, cells * 8));
    SS_TRY(dev.get(&d_dv, cells * 8));
    SS_TRY(dev.get(&d_col_slot, (size_t)n_cols * 4));
    SS_TRY(hipMemcpyAsync(d_col_slot, col_slot.data(), (size_t)n_cols * 4, hipMemcpyHostToDevice, st));
    SS_TRY(hipStreamSynchronize(st));          // (col_slot is the caller's)
    return MIDAS_SNPS_OK;
  }

  hipError_t lap(int a, int b, int slot) { return ev.lap(a, b, &ms[slot]); }

  // upload the next chunk of one matrix and index its lines (text_rows.h)
  int32_t load_chunk(Chunk& c) { return chunk_load(ctx, st, ev, c, chunk_bytes, G, d_scratch, &ms[1]); }

  // the next group: *g_out complete rows of both matrices parsed into d_fv / d_dv, or 0 when the rows are used up
  int32_t next(long long* g_out) {
    *g_out = 0;
    while (base < n_sites_max) {
      // ---- the group's rows: complete lines of both chunks ----------------------------------------------------------------
      const auto t_load = std::chrono::steady_clock::now();
      for (Chunk& c : ck) {
        int32_t rc = load_chunk(c);
        if (rc != MIDAS_SNPS_OK) return rc;
      }
      // (host clock around copies that end in a synchronise: upload + index of both chunks; the index alone is ms[1])
      ms[0] += std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_load).count();
      const long long g = std::min(std::min(ck[0].lines, ck[1].lines), std::min(G, n_sites_max - base));
      if (g == 0) {
        bool grow = false;
        for (Chunk& c : ck)
          if (c.lines == 0 && !c.at_eof) grow = true;
        if (!grow) return MIDAS_SNPS_OK;     // one of the matrices has no row left: the reference stops here too
        if (chunk_bytes >= kChunkMax) return ss_fail(ctx, MIDAS_SNPS_ERR_UNSUPPORTED, "a matrix row longer than 1 GiB");
        chunk_bytes = std::min(kChunkMax, chunk_bytes * 2);
        for (Chunk& c : ck) {
          int32_t rc = alloc_chunk(c, chunk_bytes);
          if (rc != MIDAS_SNPS_OK) return rc;
        }
        continue;
      }
      ++groups;
      // ---- parse ---------------------------------------------------------------------------------------------------------
      SS_TRY(hipEventRecord(ev.e[2], st));
      for (int m = 0; m < 2; ++m) {
        Chunk& c = ck[m];
        SS_TRY(hipMemsetAsync(c.d_side_n, 0, 4, st));
        SS_TRY(hipMemsetAsync(c.d_bad, 0xFF, 8, st));
        ParseP pp;
        pp.text = c.d_text; pp.ends = c.d_ends; pp.g = g; pp.stride = G; pp.col_slot = d_col_slot; pp.n_cols = n_cols;
        pp.val = m == 0 ? (void*)d_fv : (void*)d_dv; pp.side = c.d_side; pp.side_n = c.d_side_n; pp.side_cap = (uint32_t)cells;
        pp.bad = c.d_bad;
        if (m == 0) hipLaunchKernelGGL(ss_parse_kernel<false>, dim3(nblocks(g, 256)), dim3(256), 0, st, pp);
        else hipLaunchKernelGGL(ss_parse_kernel<true>, dim3(nblocks(g, 256)), dim3(256), 0, st, pp);
        SS_TRY(hipGetLastError());
      }
      SS_TRY(hipEventRecord(ev.e[3], st));
      uint32_t side_n[2] = {0, 0};
      end_at[0] = end_at[1] = 0;
      bad[0] = bad[1] = kNoBad;
      for (int m = 0; m < 2; ++m) {
        SS_TRY(hipMemcpyAsync(&side_n[m], ck[m].d_side_n, 4, hipMemcpyDeviceToHost, st));
        SS_TRY(hipMemcpyAsync(&bad[m], ck[m].d_bad, 8, hipMemcpyDeviceToHost, st));
        SS_TRY(hipMemcpyAsync(&end_at[m], ck[m].d_ends + g - 1, 4, hipMemcpyDeviceToHost, st));
      }
      SS_TRY(hipStreamSynchronize(st));
      SS_TRY(lap(2, 3, 2));
      // ---- the side lists: cells off the fast path, converted by the host's exact parser and patched in ----------------------
      for (int m = 0; m < 2; ++m) {
        const uint32_t n = side_n[m];
        stats[2 + m] += n;
        if (n == 0) continue;
        side_h.resize(n);
        SS_TRY(hipMemcpy(side_h.data(), ck[m].d_side, (size_t)n * sizeof(SideCell), hipMemcpyDeviceToHost));
        patch_at.clear(); patch_f.clear(); patch_i.clear();
        const char* text = ck[m].host + ck[m].at;
        for (const SideCell& sc : side_h) {
          // (a cell that starts at the appended terminator of an unterminated last line is empty: off + len stays inside)
          const std::string_view cell(text + sc.off, sc.len);
          bool ok;
          double vf = 0.0;
          int64_t vi = 0;
          if (m == 0) ok = parse_f64_py(cell, &vf);
          else ok = parse_i64_py(cell, &vi);
          if (!ok) {
            bad[m] = std::min(bad[m], ((unsigned long long)sc.row << 32) | (sc.slot + 1ull));
            continue;
          }
          patch_at.push_back((long long)sc.slot * G + sc.row);
          if (m == 0) patch_f.push_back(vf); else patch_i.push_back((long long)vi);
        }
        const size_t np = patch_at.size();
        if (np == 0) continue;
        if (np > patch_cap) {
          patch_cap = std::max(np, patch_cap * 2);
          SS_TRY(dev.get(&d_patch_at, patch_cap * 8));
          SS_TRY(dev.get((char**)&d_patch_v, patch_cap * 8));
        }
        SS_TRY(hipMemcpyAsync(d_patch_at, patch_at.data(), np * 8, hipMemcpyHostToDevice, st));
        SS_TRY(hipMemcpyAsync(d_patch_v, m == 0 ? (const void*)patch_f.data() : (const void*)patch_i.data(), np * 8, hipMemcpyHostToDevice, st));
        if (m == 0) hipLaunchKernelGGL(ss_patch_kernel<double>, dim3(nblocks((long long)np, 256)), dim3(256), 0, st, d_fv, d_patch_at, (const double*)d_patch_v, (long long)np);
        else hipLaunchKernelGGL(ss_patch_kernel<long long>, dim3(nblocks((long long)np, 256)), dim3(256), 0, st, d_dv, d_patch_at, (const long long*)d_patch_v, (long long)np);
        SS_TRY(hipGetLastError());
        SS_TRY(hipStreamSynchronize(st));       // (the host vectors are reused by the other matrix)
      }
      *g_out = g;
      return MIDAS_SNPS_OK;
    }
    return MIDAS_SNPS_OK;
  }

  // a short row or a cell that is no number among the first read_rows rows of the group: the error, with its place in stats
  int32_t check_rows(long long read_rows) {
    static const char* kFile[2] = {"freq", "depth"};
    // (the reference converts row by row, sample by sample, the frequency before the depth: the smaller key first)
    for (int m = bad[1] < bad[0] ? 1 : 0, k = 0; k < 2; ++k, m ^= 1) {
      if (bad[m] == kNoBad || (long long)(bad[m] >> 32) >= read_rows) continue;
      const long long row = base + (long long)(bad[m] >> 32);
      const long long slot = (long long)(bad[m] & 0xFFFFFFFFull) - 1;
      stats[4] = m + 1;
      stats[5] = row;
      stats[6] = slot;
      stats[0] = base;
      char buf[160];
      if (slot < 0) snprintf(buf, sizeof buf, "%s matrix, data row %lld: fewer than %d sample columns", kFile[m], row, n_cols);
      else snprintf(buf, sizeof buf, "%s matrix, data row %lld, sample %lld: not a number", kFile[m], row, slot);
      return ss_fail(ctx, MIDAS_SNPS_ERR_BAD_LAYOUT, buf);
    }
    return MIDAS_SNPS_OK;
  }

  // the first of the group's first read_rows rows that is short or holds a cell that is no number; -1: none
  long long first_bad_row(long long read_rows) const {
    long long row = -1;
    for (int m = 0; m < 2; ++m) {
      if (bad[m] == kNoBad || (long long)(bad[m] >> 32) >= read_rows) continue;
      if (row < 0 || (long long)(bad[m] >> 32) < row) row = (long long)(bad[m] >> 32);
    }
    return row;
  }

  // the group is done with: the next one starts behind its last row
  void advance(long long g) {
    base += g;
    for (int m = 0; m < 2; ++m) ck[m].at = std::min(ck[m].bytes, ck[m].at + (long long)end_at[m] + 1);
  }

  // max_sites was filled by the last row of the group just done with: the one row more that the reference converts (and then
  // stops at) opens the next group
  int32_t check_row_behind() {
    long long g = 0;
    const int32_t rc = next(&g);
    if (rc != MIDAS_SNPS_OK || g == 0) return rc;
    return check_rows(1);
  }
};

// The reference converts a row's cells and then calls the site, row by row: of a row that cannot be read and a site that
// cannot be called, the one it meets first is the error, whatever the row groups are (a row with both: the cells come first).
bool call_error_comes_first(const RowGroups& rg, long long g, unsigned long long err) {
  if (err == kNoBad) return false;
  const long long bad_row = rg.first_bad_row(g);
  return bad_row < 0 || (long long)(err >> 32) < bad_row;
}

// the statistics every walk closes with ([1], [8] and [11..13] are the entry point's own), and its phase times
void sites_end(const RowGroups& rg, float* out_ms8) {
  rg.stats[0] = rg.base;
  rg.stats[7] = rg.groups;
  rg.stats[9] = rg.G;
  rg.stats[10] = rg.chunk_bytes;
  if (out_ms8) for (int k = 0; k < 8; ++k) out_ms8[k] = rg.ms[k];
}

}  // namespace
}  // namespace midas
