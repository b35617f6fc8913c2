// What genes_compare.hip and genes_linkage.hip share: the mapped genes_<kind>.txt (midas_genes_matrix), the message of a failure
// on it, and the row parser of a chunk of its text (one thread a row, the cells converted as pandas' C reader converts them,
// sample-major).  The chunk, its newline index and the buffer holders are text_rows.h's.  Everything but the handle's type has
// internal linkage: each of the files compiles its own copy.
#pragma once
#include <sys/mman.h>

#include <cstdio>
#include <string>
#include <vector>

#include "../../include/midas_snps.h"
#include "ctx_internal.h"
#include "kernels.h"
#include "pandas_f64.h"
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

// ---- the host side of the matrix file ------------------------------------------------------------------------------------------
void gm_fail(char* err1024, const std::string& path, long long line, const char* what) {
  if (!err1024) return;
  if (line > 0) snprintf(err1024, 1024, "%s, line %lld: %s", path.c_str(), line, what);
  else snprintf(err1024, 1024, "%s: %s", path.c_str(), what);
}

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
