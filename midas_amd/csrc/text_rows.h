// The text-matrix walkers' parts that sites_rows.h (RowGroups) and genes_rows.h (GeneRows) share: a run of bytes of a
// tab-separated matrix uploaded as a chunk, its newline index (newlines counted per 16 bytes, the library's exclusive scan,
// newline k's position -> ends[k]), the device buffer and event holders, the tiles of sample pairs every pair kernel is launched
// over (pair_tiles, pair_tile), and the popcount pair kernel over a bit matrix [sample][64 rows a word].  The kernels that make
// such bit matrices are bit_planes.h's; the sizes of a walk are row_group_plan.h's.
// species_hits.hip and species_merge.hip take the index kernels and the exact one-multiply float() decoder from here too.
// Everything has internal linkage: each of the files compiles its own copy.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <vector>

#include "../../include/midas_snps.h"
#include "ctx_internal.h"
#include "kernels.h"

namespace midas {
namespace {

struct SideCell { uint32_t row, slot, off, len; };

constexpr unsigned long long kNoBad = ~0ull;

__device__ __forceinline__ uint32_t newline_bytes(uint32_t w) {     // 0x80 in every byte of w that is '\n'
  const uint32_t x = w ^ 0x0A0A0A0Au;
  return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);
}

// text is padded with zero bytes to n16 * 16
__global__ __launch_bounds__(256) void ss_count_kernel(const uint4* text, long long n16, uint32_t* counts) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n16) return;
  const uint4 v = text[i];
  counts[i] = __popc(newline_bytes(v.x)) + __popc(newline_bytes(v.y)) + __popc(newline_bytes(v.z)) + __popc(newline_bytes(v.w));
}

// ends[k] = offset of newline k, for k < cap
__global__ __launch_bounds__(256) void ss_ends_kernel(const uint4* text, long long n16, const uint32_t* prefix, uint32_t cap, uint32_t* ends) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n16) return;
  const uint4 v = text[i];
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
  uint32_t k = prefix[i];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    uint32_t m = newline_bytes(w[q]);
    while (m) {
      const int b = __ffs(m) - 1;          // bit 7, 15, 23 or 31
      if (k < cap) ends[k] = (uint32_t)(16 * i + 4 * q + (b >> 3));
      ++k;
      m &= m - 1;
    }
  }
}

// float(text) when the literal is [sign] digits [. digits] [e [sign] digits] with at most 15 significant digits and a decimal
// exponent within +-22: the digits are an exact integer below 2^53 and 10^|e| is exact, so one multiply or divide rounds once
__host__ __device__ inline bool sp_f64_fast(const char* s, uint32_t n, double* out) {
  const double p10[23] = {1e0, 1e1, 1e2, 1e3, 1e4, 1e5, 1e6, 1e7, 1e8, 1e9, 1e10, 1e11, 1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};
  uint32_t i = 0;
  bool neg = false;
  if (i < n && (s[i] == '+' || s[i] == '-')) { neg = s[i] == '-'; ++i; }
  unsigned long long m = 0;
  int sig = 0, digits = 0, frac = 0;
  bool dot = false;
  for (; i < n; ++i) {
    const char c = s[i];
    if (c >= '0' && c <= '9') {
      ++digits;
      if (sig > 0 || c != '0') ++sig;
      if (sig > 15) return false;
      m = m * 10 + (unsigned)(c - '0');
      if (dot) ++frac;
    } else if (c == '.' && !dot) {
      dot = true;
    } else {
      break;
    }
  }
  if (digits == 0 || frac > 400) return false;
  int ex = 0;
  if (i < n) {
    if (s[i] != 'e' && s[i] != 'E') return false;
    ++i;
    bool eneg = false;
    if (i < n && (s[i] == '+' || s[i] == '-')) { eneg = s[i] == '-'; ++i; }
    if (i >= n || n - i > 3) return false;
    for (; i < n; ++i) {
      if (s[i] < '0' || s[i] > '9') return false;
      ex = ex * 10 + (s[i] - '0');
    }
    if (eneg) ex = -ex;
  }
  const int e10 = ex - frac;
  double v = (double)m;
  if (m != 0) {
    if (e10 < -22 || e10 > 22) return false;
    v = e10 >= 0 ? v * p10[e10] : v / p10[-e10];
  }
  *out = neg ? -v : v;
  return true;
}

__device__ __forceinline__ bool is_digit(char c) { return c >= '0' && c <= '9'; }

int32_t ss_fail(midas_snps_ctx* ctx, int32_t st, const char* msg) {
  ctx->set_error(msg);
  return st;
}

#define SS_TRY(call)                                                                                             \
  do {                                                                                                           \
    hipError_t e__ = (call);                                                                                     \
    if (e__ != hipSuccess) {                                                                                     \
      char buf__[384];                                                                                           \
      snprintf(buf__, sizeof buf__, "%s: %s", #call, hipGetErrorString(e__));                                    \
      (void)hipGetLastError();                                                                                   \
      return ss_fail(ctx, e__ == hipErrorOutOfMemory ? MIDAS_SNPS_ERR_OUT_OF_MEMORY : MIDAS_SNPS_ERR_HIP, buf__); \
    }                                                                                                            \
  } while (0)

struct SsBufs {
  std::vector<void*> ptrs;
  ~SsBufs() { for (void* q : ptrs) (void)hipFree(q); }
  template <class T> hipError_t get(T** out, size_t bytes) {
    void* q = nullptr;
    const hipError_t e = hipMalloc(&q, bytes ? bytes : 16);
    if (e == hipSuccess) ptrs.push_back(q);
    *out = static_cast<T*>(q);
    return e;
  }
};

struct SsEvents {
  hipEvent_t e[8] = {};
  ~SsEvents() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
  hipError_t lap(int a, int b, float* ms) {      // *ms += the device time from e[a] to e[b]
    float t = 0.f;
    const hipError_t err = hipEventElapsedTime(&t, e[a], e[b]);
    if (err == hipSuccess) *ms += t;
    return err;
  }
};

unsigned nblocks(long long n, long long per) { return (unsigned)((n + per - 1) / per); }

// one matrix's chunk on the device: the text, its newline index
struct Chunk {
  const char* host = nullptr;
  long long bytes = 0, at = 0;   // the file's body, where the next group starts
  char* d_text = nullptr;
  uint32_t* d_counts = nullptr;
  uint32_t* d_ends = nullptr;
  SideCell* d_side = nullptr;
  uint32_t* d_side_n = nullptr;
  unsigned long long* d_bad = nullptr;
  long long n = 0;               // bytes of the chunk on the device (a final line without '\n' got one)
  long long lines = 0;
  bool at_eof = false;
};

// the pair kernel's tile (strain_tracking.py track_markers, compare_genes.py --dtype presabs)
constexpr int kPairTile = MIDAS_SITES_PAIR_TILE;      // samples a side of a workgroup's tile of pairs
constexpr int kPairRun = 32;                          // words of every sample staged at a time
constexpr int kPairPad = kPairTile + 1;               // the staged words lie [word][sample]: 65 keeps the transposing stores apart

// The tiles of `tile` samples a side on or above the diagonal of the S x S pairs, counted row by row: a pair kernel's blockIdx.x
struct PairTiles { int side; long long n; };
PairTiles pair_tiles(int S, int tile) {
  const int side = (S + tile - 1) / tile;
  return PairTiles{side, (long long)side * (side + 1) / 2};
}
struct PairTile { int ti, tj; };                      // ti <= tj
__device__ __forceinline__ PairTile pair_tile(int block, int tiles_side) {
  int ti = 0, left = block;
  while (left >= tiles_side - ti) { left -= tiles_side - ti; ++ti; }
  return PairTile{ti, ti + left};
}
// both[i][j] += sum over words of popcount(B[i][w] & B[j][w]) for i <= j.  A workgroup owns a 64 x 64 tile of pairs on or
// above the diagonal (blockIdx.x counts those tiles row by row) and a run of words (blockIdx.y); it stages 32 words of its
// two strips of samples in LDS, [word][sample], and a thread keeps a 4 x 4 part of the tile: rows ty + 16 i, columns
// tx + 16 j, so that a wave's reads of one word are 16 neighbouring columns and 4 rows (broadcast).  Sums of integers: the
// order of the groups, of the word runs and of the atomics does not matter.
__global__ __launch_bounds__(256) void ss_pairs_kernel(const unsigned long long* bits, long long wstride, long long n_words, long long run_words,
                                                       int S, int tiles_side, unsigned long long* both) {
  __shared__ unsigned long long sa[kPairRun][kPairPad], sb[kPairRun][kPairPad];
  const PairTile tile = pair_tile(blockIdx.x, tiles_side);
  const int ti = tile.ti, tj = tile.tj;
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const long long w0 = (long long)blockIdx.y * run_words, w1 = w0 + run_words < n_words ? w0 + run_words : n_words;
  uint32_t sum[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) sum[i][j] = 0;
  for (long long k0 = w0; k0 < w1; k0 += kPairRun) {
#pragma unroll
    for (int it = 0; it < kPairTile * kPairRun / 256; ++it) {
      const int e = it * 256 + tid, s = e / kPairRun, k = e % kPairRun;
      const long long w = k0 + k;
      const int gi = ti * kPairTile + s, gj = tj * kPairTile + s;
      sa[k][s] = (gi < S && w < w1) ? bits[(long long)gi * wstride + w] : 0ull;
      sb[k][s] = (gj < S && w < w1) ? bits[(long long)gj * wstride + w] : 0ull;
    }
    __syncthreads();
#pragma unroll 4
    for (int k = 0; k < kPairRun; ++k) {
      unsigned long long a[4], b[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) { a[i] = sa[k][ty + 16 * i]; b[i] = sb[k][tx + 16 * i]; }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) sum[i][j] += (uint32_t)__popcll(a[i] & b[j]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int gi = ti * kPairTile + ty + 16 * i, gj = tj * kPairTile + tx + 16 * j;
      if (gi <= gj && gj < S && sum[i][j]) atomicAdd(&both[(long long)gi * S + gj], (unsigned long long)sum[i][j]);
    }
}

// The word runs of a pair kernel's launch (its blockIdx.y): enough workgroups to fill the device when the tiles are few --
// pair_blocks is the aim -- each run whole staging steps of `step` words (kPairRun, or the planes' own)
struct PairRuns { long long runs, run_words; };
PairRuns pair_runs(long long n_words, long long n_tiles, long long pair_blocks, int step) {
  long long runs = std::max<long long>(1, std::min<long long>((pair_blocks + n_tiles - 1) / n_tiles, (n_words + step - 1) / step));
  runs = std::min<long long>(runs, 65535);
  const long long run_words = ((n_words + runs - 1) / runs + step - 1) / step * step;
  return PairRuns{(n_words + run_words - 1) / run_words, run_words};
}

// device room for a chunk of cb bytes (the text padded to 16 and one terminator, the per-16-byte newline counts)
int32_t chunk_alloc(midas_snps_ctx* ctx, SsBufs& dev, Chunk& c, long long cb) {
  const size_t padded = ((size_t)cb + 1 + 15) / 16 * 16;
  SS_TRY(dev.get(&c.d_text, padded));
  SS_TRY(dev.get(&c.d_counts, padded / 16 * 4));
  return MIDAS_SNPS_OK;
}

// upload the next chunk_bytes of a matrix and index its lines: c.lines complete lines, the first `cap` of them in c.d_ends.
// ev.e[1] / e[2] bracket the index; its device time is added to *index_ms
int32_t chunk_load(midas_snps_ctx* ctx, hipStream_t st, SsEvents& ev, Chunk& c, long long chunk_bytes, long long cap, uint32_t* d_scratch,
                   float* index_ms) {
  const long long left = c.bytes - c.at;
  long long n = std::min(left, chunk_bytes);
  c.at_eof = n == left;
  if (n > 0) SS_TRY(hipMemcpyAsync(c.d_text, c.host + c.at, (size_t)n, hipMemcpyHostToDevice, st));
  if (c.at_eof && n > 0 && c.host[c.at + n - 1] != '\n') {      // the last line has no terminator: it is a row all the same
    const char nl = '\n';
    SS_TRY(hipMemcpyAsync(c.d_text + n, &nl, 1, hipMemcpyHostToDevice, st));
    ++n;
  }
  const long long n16 = (n + 15) / 16;
  if (n16 * 16 > n) SS_TRY(hipMemsetAsync(c.d_text + n, 0, (size_t)(n16 * 16 - n), st));
  c.n = n;
  c.lines = 0;
  if (n == 0) return MIDAS_SNPS_OK;
  SS_TRY(hipEventRecord(ev.e[1], st));
  hipLaunchKernelGGL(ss_count_kernel, dim3(nblocks(n16, 256)), dim3(256), 0, st, (const uint4*)c.d_text, n16, c.d_counts);
  SS_TRY(hipGetLastError());
  uint32_t last_count = 0, last_prefix = 0;
  SS_TRY(hipMemcpyAsync(&last_count, c.d_counts + n16 - 1, 4, hipMemcpyDeviceToHost, st));
  SS_TRY(launch_scan_u32(c.d_counts, c.d_counts, n16, d_scratch, st));
  SS_TRY(hipMemcpyAsync(&last_prefix, c.d_counts + n16 - 1, 4, hipMemcpyDeviceToHost, st));
  hipLaunchKernelGGL(ss_ends_kernel, dim3(nblocks(n16, 256)), dim3(256), 0, st, (const uint4*)c.d_text, n16, c.d_counts, (uint32_t)cap,
                     c.d_ends);
  SS_TRY(hipGetLastError());
  SS_TRY(hipEventRecord(ev.e[2], st));
  SS_TRY(hipStreamSynchronize(st));
  SS_TRY(ev.lap(1, 2, index_ms));
  c.lines = (long long)last_count + last_prefix;
  return MIDAS_SNPS_OK;
}

}  // namespace
}  // namespace midas
