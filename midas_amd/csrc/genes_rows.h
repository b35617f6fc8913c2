// What the commands over genes_<kind>.txt share (genes_compare.hip, genes_linkage.hip): the mapped file (midas_genes_matrix) and
// the message of a failure on it, the row parser of a chunk of its text (one thread a row, the cells converted as pandas' C reader
// converts them, sample-major), the walker that takes the text through that parser a row group at a time (genes_begin, GeneRows:
// the shape of RowGroups in sites_rows.h, for one matrix and without a side list), and the buffered writer of the output
// tables (TableWriter).  The chunk, its newline index, the buffer and event holders and the pair tiles are text_rows.h's, the
// sizes of the walk row_group_plan.h's, the bit planes bit_planes.h's.  Everything but the handle's type has internal linkage:
// each of the files compiles its own copy.
#pragma once
#include <sys/mman.h>

#include <algorithm>
#include <charconv>
#include <chrono>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/midas_snps.h"
#include "bit_planes.h"
#include "ctx_internal.h"
#include "kernels.h"
#include "pandas_f64.h"
#include "row_group_plan.h"
#include "text_rows.h"

namespace midas {
namespace {

struct GcParseP {
  const char* text;            // the chunk
  const uint32_t* ends;        // newline offsets of its rows
  long long g, stride;         // rows to parse; row stride of a sample's values
  int S, n_cols;               // sample columns converted (the first S); sample columns a row must have
  double* val;                 // [S][stride]
  uint32_t* col_float;         // [S] set when a cell of the column has '.' or an exponent
  unsigned long long* bad;     // min over (row << 32 | column + 1); column + 1 == 0: the row has another width
};

__global__ __launch_bounds__(256) void gc_parse_kernel(GcParseP p) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r >= p.g) return;
  const uint32_t b = r == 0 ? 0u : p.ends[r - 1] + 1u;
  uint32_t e = p.ends[r];
  const char* t = p.text;
  if (e > b && t[e - 1] == '\r') --e;
  uint32_t q = b;
  while (q < e && t[q] != '\t') ++q;         // the gene id
  int c = 0;
  while (q < e) {                            // t[q] is the tab in front of sample column c
    const uint32_t fs = ++q;
    while (q < e && t[q] != '\t') ++q;
    if (c < p.S) {
      double v = 0.0;
      bool plain_int = true;
      if (!pandas_f64(t + fs, (int)(q - fs), &v, &plain_int)) atomicMin(p.bad, ((unsigned long long)r << 32) | (unsigned long long)(c + 1));
      else if (!plain_int) p.col_float[c] = 1u;
      p.val[(long long)c * p.stride + r] = v;
    }
    ++c;
  }
  if (c != p.n_cols) atomicMin(p.bad, (unsigned long long)r << 32);
}

// What every entry point over the matrix checks alike, after the checks that are its own: the text, the row, sample and column
// counts, group_rows and chunk_bytes (iparams[0], [1]) and the statistics array; then the context's error and the caller's
// statistics and times are reset.
int32_t genes_begin(midas_snps_ctx* ctx, const char* text, int64_t text_bytes, int64_t n_rows_max, int32_t n_samples, int32_t n_columns,
                    const int64_t* iparams, int64_t* out_stats16, float* out_ms8) {
  if (!ctx || text_bytes < 0 || (text_bytes > 0 && !text) || n_rows_max < 0 || n_samples < 1 || n_columns < n_samples || !iparams ||
      !out_stats16 || iparams[0] < 0 || iparams[1] < 0)
    return MIDAS_SNPS_ERR_INVALID_ARG;
  ctx->clear_error();
  ctx->err_read = -1;
  for (int k = 0; k < 16; ++k) out_stats16[k] = 0;
  out_stats16[5] = -1;
  out_stats16[6] = -1;
  if (out_ms8) for (int k = 0; k < 8; ++k) out_ms8[k] = 0.f;
  return MIDAS_SNPS_OK;
}

// The rows of the matrix on the device, a group at a time: upload, line index, cell parse.  next() leaves the group's cells in
// d_val, [sample][G], and the parse queued; the caller queues its own kernels behind it, then check() waits for all of it and
// turns a bad row into the error, and advance() moves on.
// The events and the times they give.  Here: e[1] -> e[2] the index (chunk_load) -> ms[1]; e[2] -> e[3] the parse -> ms[2];
// ms[0] is the host clock around upload + index.  The caller's: e[3] (the parse's end) -> e[4] -> e[5] its kernels on a group ->
// ms[3], ms[4]; behind the walk e[0] -> e[1] (and e[2] -> e[3]) whatever runs once -> ms[4 .. 6], and the download -> ms[7].
struct GeneRows {
  midas_snps_ctx* ctx;
  hipStream_t st;
  SsBufs& dev;
  SsEvents& ev;
  float* ms;
  int64_t* stats;                // the caller's out_stats16: [0], [4..6] on a bad row; [0], [7], [9], [10] at the end
  int S = 0, n_cols = 0;
  long long G = 0, chunk_bytes = 0, n_rows_max = 0;
  Chunk ck;
  uint32_t* d_scratch = nullptr;
  uint32_t* d_col_float = nullptr;
  double* d_val = nullptr;
  long long base = 0, groups = 0;
  uint32_t end_at = 0;           // offset of the newline of the group's last row

  GeneRows(midas_snps_ctx* c, SsBufs& d, SsEvents& e, float* ms8, int64_t* stats16) : ctx(c), st(c->stream), dev(d), ev(e), ms(ms8), stats(stats16) {}

  // sizes: rows a group (G) and bytes a chunk, from the caller or from a quarter of the free device memory; per_row = the
  // device bytes a row of the group takes in the caller's and in these buffers; scan_items = the most items the caller scans
  // with d_scratch
  int32_t init(const char* text, long long text_bytes, long long n_max, int n_samples, int n_columns, long long G_in, long long chunk_in,
               long long per_row, long long scan_items) {
    S = n_samples;
    n_cols = n_columns;
    n_rows_max = n_max;
    size_t free_b = 0, total_b = 0;
    if (G_in == 0 || chunk_in == 0) SS_TRY(hipMemGetInfo(&free_b, &total_b));
    const RowGroupPlan plan = plan_row_groups(free_b, G_in, chunk_in, 1, text_bytes, n_rows_max, per_row);
    G = plan.G;
    chunk_bytes = plan.chunk_bytes;
    const size_t cells = (size_t)G * (size_t)S;
    if (cells > 0xFFFFFFF0ull) return ss_fail(ctx, MIDAS_SNPS_ERR_UNSUPPORTED, "a row group beyond 2^32 cells: lower group_rows");
    for (auto& x : ev.e) SS_TRY(hipEventCreate(&x));
    ck.host = text;
    ck.bytes = text_bytes;
    const int32_t rc = chunk_alloc(ctx, dev, ck, chunk_bytes);
    if (rc != MIDAS_SNPS_OK) return rc;
    SS_TRY(dev.get(&ck.d_ends, ((size_t)G + 1) * 4));
    SS_TRY(dev.get(&ck.d_bad, 8));
    SS_TRY(dev.get(&d_scratch, scan_scratch_words(std::max<long long>((kChunkMax + 16) / 16, scan_items)) * 4));
    SS_TRY(dev.get(&d_val, cells * 8));
    SS_TRY(dev.get(&d_col_float, (size_t)S * 4));
    SS_TRY(hipMemsetAsync(d_col_float, 0, (size_t)S * 4, st));
    return MIDAS_SNPS_OK;
  }

  hipError_t lap(int a, int b, int slot) { return ev.lap(a, b, &ms[slot]); }

  // the next group: *g_out complete rows uploaded, indexed and their parse queued (e[2] .. e[3]), or 0 when the rows are used up
  int32_t next(long long* g_out) {
    *g_out = 0;
    while (base < n_rows_max) {
      const auto t_load = std::chrono::steady_clock::now();
      int32_t rc = chunk_load(ctx, st, ev, ck, chunk_bytes, G, d_scratch, &ms[1]);
      if (rc != MIDAS_SNPS_OK) return rc;
      ms[0] += std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_load).count();
      const long long g = std::min(ck.lines, std::min(G, n_rows_max - base));
      if (g == 0) {
        if (ck.at_eof) return MIDAS_SNPS_OK;
        if (chunk_bytes >= kChunkMax) return ss_fail(ctx, MIDAS_SNPS_ERR_UNSUPPORTED, "a matrix row longer than 1 GiB");
        chunk_bytes = std::min(kChunkMax, chunk_bytes * 2);
        rc = chunk_alloc(ctx, dev, ck, chunk_bytes);
        if (rc != MIDAS_SNPS_OK) return rc;
        continue;
      }
      ++groups;
      SS_TRY(hipMemsetAsync(ck.d_bad, 0xFF, 8, st));
      SS_TRY(hipEventRecord(ev.e[2], st));
      GcParseP pp;
      pp.text = ck.d_text; pp.ends = ck.d_ends; pp.g = g; pp.stride = G; pp.S = S; pp.n_cols = n_cols; pp.val = d_val;
      pp.col_float = d_col_float; pp.bad = ck.d_bad;
      hipLaunchKernelGGL(gc_parse_kernel, dim3(nblocks(g, 256)), dim3(256), 0, st, pp);
      SS_TRY(hipGetLastError());
      SS_TRY(hipEventRecord(ev.e[3], st));
      *g_out = g;
      return MIDAS_SNPS_OK;
    }
    return MIDAS_SNPS_OK;
  }

  // waits for the group's work, the caller's behind the parse included; a row of another width or a cell that is no number is
  // the error, with its place in stats
  int32_t check(long long g) {
    unsigned long long bad = kNoBad;
    SS_TRY(hipMemcpyAsync(&bad, ck.d_bad, 8, hipMemcpyDeviceToHost, st));
    SS_TRY(hipMemcpyAsync(&end_at, ck.d_ends + g - 1, 4, hipMemcpyDeviceToHost, st));
    SS_TRY(hipStreamSynchronize(st));
    SS_TRY(lap(2, 3, 2));
    if (bad == kNoBad) return MIDAS_SNPS_OK;
    // (the groups come in file order and a group reports its earliest: the file's earliest)
    const long long row = base + (long long)(bad >> 32), col = (long long)(bad & 0xFFFFFFFFull) - 1;
    stats[0] = base;
    stats[4] = col < 0 ? 1 : 2;
    stats[5] = row;
    stats[6] = col;
    char buf[160];
    if (col < 0) snprintf(buf, sizeof buf, "data row %lld: not %d sample columns wide", row, n_cols);
    else snprintf(buf, sizeof buf, "data row %lld, sample column %lld: not a finite decimal number", row, col);
    return ss_fail(ctx, MIDAS_SNPS_ERR_BAD_LAYOUT, buf);
  }

  // the group is done with: the next one starts behind its last row
  void advance(long long g) {
    base += g;
    ck.at = std::min(ck.bytes, ck.at + (long long)end_at + 1);
  }

  // the statistics every walk closes with ([1], [8] and [11..14] are the entry point's own), and its phase times
  void end(float* out_ms8) {
    stats[0] = base;
    stats[7] = groups;
    stats[9] = G;
    stats[10] = chunk_bytes;
    if (out_ms8) for (int k = 0; k < 8; ++k) out_ms8[k] = ms[k];
  }
};

// ---- the host side of the matrix file ------------------------------------------------------------------------------------------
void gm_fail(char* err1024, const std::string& path, long long line, const char* what) {
  if (!err1024) return;
  if (line > 0) snprintf(err1024, 1024, "%s, line %lld: %s", path.c_str(), line, what);
  else snprintf(err1024, 1024, "%s: %s", path.c_str(), what);
}

// An output table written through a 1 MiB buffer: the caller appends to buf, numbers through i64 / f64 (as str() writes them), and
// closes a row with row_done().  f is null when the file cannot be opened; a failed write or fclose makes close() false.
struct TableWriter {
  FILE* f = nullptr;
  std::string buf;
  bool ok = true;
  explicit TableWriter(const char* path) : f(fopen(path, "w")) { buf.reserve(1 << 20); }
  void i64(int64_t v) {
    char tmp[24];
    buf.append(tmp, (size_t)(std::to_chars(tmp, tmp + sizeof tmp, v).ptr - tmp));
  }
  void f64(double v) {
    char tmp[40];
    int64_t n = 0;
    midas_genes_merge_format_f64(1, &v, tmp, sizeof tmp, &n);
    buf.append(tmp, (size_t)(n > 0 ? n - 1 : 0));      // (without the formatter's '\n')
  }
  void row_done() {
    buf.push_back('\n');
    if (buf.size() > (1u << 20) - 4096) {
      ok = fwrite(buf.data(), 1, buf.size(), f) == buf.size() && ok;
      buf.clear();
    }
  }
  bool close() {
    ok = (buf.empty() || fwrite(buf.data(), 1, buf.size(), f) == buf.size()) && ok;
    ok = fclose(f) == 0 && ok;
    f = nullptr;
    return ok;
  }
};

}  // namespace
}  // namespace midas

struct midas_genes_matrix {
  std::string path;
  const char* base = nullptr;
  size_t size = 0, body = 0;          // the mapping; offset of the first byte after the header line
  std::vector<char> id_pool;          // the header's fields after the first, back to back
  std::vector<int64_t> id_off{0};
  std::string first_field;
  int64_t n_rows = 0;
  ~midas_genes_matrix() { if (base && size) munmap(const_cast<char*>(base), size); }
};
