// Bit planes from the parsed cells of a row group, [sample][stride]: the two kernels that turn a yes / no a (row, sample) into
// 64-bit words, and the two cells they are built for.
//   planes_by_row_kernel      row-major planes [row][W], a word = 64 samples (gene_linkage.py, snp_ld.py)
//   planes_by_sample_kernel   sample-major planes [sample][wstride], a word = 64 rows (compare_genes.py, snp_trees.py)
// A cell is a functor: row(k) = the group's row behind the k-th row of the planes (itself, or list[k] where only retained rows get
// a place), bits(row, s) = bit p set: the cell belongs to plane p.  kPlanes = 1 or 2 planes are written.
// sites_ld.hip, sites_trees.hip and genes_compare.hip are compiled with -ffp-contract=off, genes_linkage.hip without it
// (build.py): nothing here may depend on that flag, so this file holds no floating-point arithmetic, only comparisons.
// Everything has internal linkage: each of the files compiles its own copy.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace midas {
namespace {

// plane 0: value > cutoff (the gene is present in the sample)
struct PresentCell {
  const double* val;           // [S][stride]
  long long stride;
  double cutoff;
  __device__ long long row(long long k) const { return k; }
  __device__ unsigned bits(long long row, int s) const { return val[(long long)s * stride + row] > cutoff ? 1u : 0u; }
};

// plane 0 `called`: where ss_seq_kernel writes a letter (the cell is kept and depth != 0); plane 1 `minor`: that letter is the
// minor allele (freq >= 0.5).  list: retained site k of the group -> its row
struct ConsensusCell {
  const double* fv;            // [S][stride]
  const long long* dv;         // [S][stride]
  const uint8_t* cell;         // [S][stride] bit 0: the sample is kept at the site
  const uint32_t* list;
  long long stride;
  __device__ long long row(long long k) const { return (long long)list[k]; }
  __device__ unsigned bits(long long row, int s) const {
    const long long at = (long long)s * stride + row;
    if (!((cell[at] & 1) && dv[at] != 0)) return 0u;
    return fv[at] >= 0.5 ? 3u : 1u;
  }
};

// The planes of m rows, [row][W words]: blockIdx.x = 64 rows, blockIdx.y = the word (64 samples).  Wave v ballots the samples
// 16 v .. 16 v + 15 of the word, a lane a row (the reads run along the rows, as the cells lie); then thread t < 64 gathers bit t
// of the 64 sample words: the 64 x 64 bit block is turned in LDS.  The pad bits of the last word are 0.
template <int kPlanes, class Cell>
__global__ __launch_bounds__(256) void planes_by_row_kernel(Cell cell, long long m, int S, int W, unsigned long long* plane0,
                                                            unsigned long long* plane1) {
  __shared__ unsigned long long t[kPlanes][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, w = blockIdx.y;
  const long long k = (long long)blockIdx.x * 64 + lane;
  const long long row = k < m ? cell.row(k) : 0;
  for (int i = 0; i < 16; ++i) {
    const int j = wave * 16 + i, s = w * 64 + j;
    const unsigned b = (k < m && s < S) ? cell.bits(row, s) : 0u;
#pragma unroll
    for (int p = 0; p < kPlanes; ++p) {
      const unsigned long long word = __ballot((b >> p) & 1u);
      if (lane == 0) t[p][j] = word;
    }
  }
  __syncthreads();
  if (threadIdx.x < 64 && k < m) {
    unsigned long long c[kPlanes];
#pragma unroll
    for (int p = 0; p < kPlanes; ++p) c[p] = 0;
#pragma unroll 8
    for (int j = 0; j < 64; ++j)
#pragma unroll
      for (int p = 0; p < kPlanes; ++p) c[p] |= ((t[p][j] >> lane) & 1ull) << j;
    plane0[k * W + w] = c[0];
    if (kPlanes > 1) plane1[k * W + w] = c[kPlanes - 1];
  }
}

// The planes of m rows, [sample][wstride words]: one wave a (sample, 64 rows), blockIdx.x = the word, blockIdx.y = 4 samples; the
// ballot is the word.
template <int kPlanes, class Cell>
__global__ __launch_bounds__(256) void planes_by_sample_kernel(Cell cell, long long m, int S, long long wstride, unsigned long long* plane0,
                                                               unsigned long long* plane1) {
  const int s = blockIdx.y * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (s >= S) return;                                  // (the whole wave)
  const long long k = (long long)blockIdx.x * 64 + lane;
  const unsigned b = k < m ? cell.bits(cell.row(k), s) : 0u;
  const unsigned long long w0 = __ballot(b & 1u), w1 = kPlanes > 1 ? __ballot(b & 2u) : 0ull;
  if (lane == 0) {
    plane0[(long long)s * wstride + blockIdx.x] = w0;
    if (kPlanes > 1) plane1[(long long)s * wstride + blockIdx.x] = w1;
  }
}

}  // namespace
}  // namespace midas
