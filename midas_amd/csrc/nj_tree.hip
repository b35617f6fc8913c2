// snp_trees.py on MI355X: neighbour joining (Saitou & Nei 1987, in Studier & Keppler's form) over a resident distance matrix.
//
// The matrix D [n][n] fp64 stays on the device; slots 0..n-1 are active, r = n.  While r > 3, four launches on one stream:
//   sums     lane = row a: R[a] = the sum of D[a][b] over the active b != a in ascending slot order, one add each from 0.0.  The
//            entries are D[b][a], down the symmetric column, so that neighbouring rows load neighbouring doubles; a workgroup
//            stages 128 of them a row through LDS, and the loads of a tile are in flight together
//   arg-min  a workgroup a row a: q = (((double)(r - 2) * D[a][b]) - R[a]) - R[b] for the active b > a, the least (q, a, b) of the
//            row -- by value, ties to the smaller a, then the smaller b: a total order on the pairs, so the minimum does not depend
//            on how it is reduced -- then one workgroup over the rows' candidates.  It leaves the chosen pair in device memory,
//            with la = 0.5 * D[a][b] + (R[a] - R[b]) / (2.0 * (double)(r - 2)) and lb = D[a][b] - la, at step n - r
//   join     lane = k: D[a][k] = D[k][a] = 0.5 * ((D[a][k] + D[b][k]) - D[a][b]) for the active k != a, b; slot b goes inactive
// and with three slots a < b < c left: la = 0.5 * ((D[a][b] + D[a][c]) - D[b][c]), lb, lc alike.  The host enqueues all n - 3
// steps and synchronises once, at the end.  Every operation is one rounded fp64 operation as written here: this file is compiled
// with -ffp-contract=off (build.py).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>

#include "../../include/midas_snps.h"
#include "ctx_internal.h"
#include "text_rows.h"

namespace midas {
namespace {

constexpr int kNoSlot = 0x7FFFFFFF;
constexpr int kSumRows = 32, kSumTile = 128;           // the row sums: rows a workgroup, column entries staged at a time

struct NjBest { double q; int a, b; };

// (q, a, b) in lexicographic order; a == kNoSlot: no candidate
__device__ __forceinline__ bool nj_before(const NjBest& x, const NjBest& y) {
  if (x.a == kNoSlot) return false;
  if (y.a == kNoSlot) return true;
  if (x.q < y.q) return true;
  if (x.q == y.q) return x.a < y.a || (x.a == y.a && x.b < y.b);
  return false;
}

// the least of the workgroup's 256 candidates, in every thread's return value
__device__ NjBest nj_block_min(NjBest mine, NjBest* sh) {
  const int tid = threadIdx.x;
  sh[tid] = mine;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (tid < h && nj_before(sh[tid + h], sh[tid])) sh[tid] = sh[tid + h];
    __syncthreads();
  }
  const NjBest out = sh[0];
  __syncthreads();
  return out;
}

// R[a] for kSumRows neighbouring rows a workgroup.  The whole workgroup stages a tile of kSumTile column entries of each of its
// rows in LDS -- D[b][a0..a0 + 31], 256 neighbouring bytes a b, sixteen loads in flight a thread, the next tile's issued before
// this tile's adds -- then lane = row adds the tile's entries in slot order: the sum is the sequential one while the loads are
// not.  An entry that does not count (slot b inactive, b == a) is added as +0.0, which keeps the select out of the chain of
// adds and changes no bit: a sum that starts from +0.0 is never -0.0, and s + 0.0 == s for every other s.
__global__ __launch_bounds__(256) void nj_sums_kernel(const double* D, const uint8_t* active, int n, double* R) {
  constexpr int kLoads = kSumTile * kSumRows / 256;
  __shared__ double tile[kSumTile][kSumRows + 1];
  __shared__ uint8_t on[kSumTile];
  const int tid = threadIdx.x, a0 = blockIdx.x * kSumRows, a = a0 + tid;
  double next[kLoads];
  auto load = [&](int b0) {
#pragma unroll
    for (int it = 0; it < kLoads; ++it) {
      const int e = it * 256 + tid, b = b0 + e / kSumRows, aa = a0 + e % kSumRows;
      next[it] = (b < n && aa < n) ? D[(long long)b * n + aa] : 0.0;
    }
  };
  load(0);
  double sum = 0.0;
  for (int b0 = 0; b0 < n; b0 += kSumTile) {
#pragma unroll
    for (int it = 0; it < kLoads; ++it) {
      const int e = it * 256 + tid;
      tile[e / kSumRows][e % kSumRows] = next[it];
    }
    if (tid < kSumTile) on[tid] = b0 + tid < n && active[b0 + tid];
    __syncthreads();
    if (b0 + kSumTile < n) load(b0 + kSumTile);
    if (tid < kSumRows) {
      for (int bb0 = 0; bb0 < kSumTile; bb0 += 16) {
        double v[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) v[j] = (on[bb0 + j] && b0 + bb0 + j != a) ? tile[bb0 + j][tid] : 0.0;
#pragma unroll
        for (int j = 0; j < 16; ++j) sum += v[j];
      }
    }
    __syncthreads();
  }
  if (tid < kSumRows && a < n && active[a]) R[a] = sum;
}

__global__ __launch_bounds__(256) void nj_row_min_kernel(const double* D, const uint8_t* active, const double* R, int n, int r, NjBest* part) {
  __shared__ NjBest sh[256];
  const int a = blockIdx.x;
  NjBest best{0.0, kNoSlot, kNoSlot};
  if (active[a]) {                                     // (the whole workgroup)
    const double scale = (double)(r - 2), ra = R[a];
    for (int b = a + 1 + threadIdx.x; b < n; b += 256) {
      if (!active[b]) continue;
      const NjBest c{((scale * D[(long long)a * n + b]) - ra) - R[b], a, b};
      if (nj_before(c, best)) best = c;
    }
  }
  best = nj_block_min(best, sh);
  if (threadIdx.x == 0) part[a] = best;
}

// one workgroup: the chosen pair of the step, its branch lengths, the record.  Without a pair (every q a NaN) the step is
// flagged and nothing is joined.
__global__ __launch_bounds__(256) void nj_choose_kernel(const double* D, const double* R, const NjBest* part, int n, int r, int step, int* pair,
                                                        int* join, double* len, int* err) {
  __shared__ NjBest sh[256];
  NjBest best{0.0, kNoSlot, kNoSlot};
  for (int a = threadIdx.x; a < n; a += 256)
    if (nj_before(part[a], best)) best = part[a];
  best = nj_block_min(best, sh);
  if (threadIdx.x != 0) return;
  pair[0] = best.a;
  pair[1] = best.b;
  if (best.a == kNoSlot) {
    *err = 1;
    return;
  }
  const double dab = D[(long long)best.a * n + best.b];
  const double la = 0.5 * dab + __ddiv_rn(R[best.a] - R[best.b], 2.0 * (double)(r - 2));
  join[2 * step] = best.a;
  join[2 * step + 1] = best.b;
  len[2 * step] = la;
  len[2 * step + 1] = dab - la;
}

__global__ __launch_bounds__(256) void nj_join_kernel(double* D, uint8_t* active, const int* pair, int n) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  const int a = pair[0], b = pair[1];
  if (k >= n || a == kNoSlot) return;
  if (k == b) { active[b] = 0; return; }               // (no other thread reads active[b] or writes row or column b)
  if (k == a || !active[k]) return;
  const double v = 0.5 * ((D[(long long)a * n + k] + D[(long long)b * n + k]) - D[(long long)a * n + b]);
  D[(long long)a * n + k] = v;
  D[(long long)k * n + a] = v;
}

__global__ void nj_last_kernel(const double* D, const uint8_t* active, int n, int* last, double* last_len, int* err) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  int s[3] = {0, 0, 0}, m = 0;
  for (int k = 0; k < n; ++k)
    if (active[k]) {
      if (m < 3) s[m] = k;
      ++m;
    }
  if (m != 3) {                                        // (a step without a pair left more than three)
    *err = 1;
    return;
  }
  const double ab = D[(long long)s[0] * n + s[1]], ac = D[(long long)s[0] * n + s[2]], bc = D[(long long)s[1] * n + s[2]];
  last[0] = s[0]; last[1] = s[1]; last[2] = s[2];
  last_len[0] = 0.5 * ((ab + ac) - bc);
  last_len[1] = 0.5 * ((ab + bc) - ac);
  last_len[2] = 0.5 * ((ac + bc) - ab);
}

}  // namespace
}  // namespace midas

using namespace midas;

extern "C" int32_t midas_nj_tree(midas_snps_ctx* ctx, int32_t n, const double* dist, int32_t* out_join, double* out_len, int32_t* out_last,
                                 double* out_last_len, int64_t* out_stats16, float* out_ms8) {
  if (!ctx || n < 3 || !dist || !out_last || !out_last_len || !out_stats16 || (n > 3 && (!out_join || !out_len)))
    return MIDAS_SNPS_ERR_INVALID_ARG;
  ctx->clear_error();
  for (int k = 0; k < 16; ++k) out_stats16[k] = 0;
  if (out_ms8) for (int k = 0; k < 8; ++k) out_ms8[k] = 0.f;
  const size_t nn = (size_t)n * (size_t)n;
  for (size_t k = 0; k < nn; ++k)
    if (!std::isfinite(dist[k])) return ss_fail(ctx, MIDAS_SNPS_ERR_INVALID_ARG, "the distance matrix holds a value that is not finite");
  SS_TRY(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  {
    size_t free_b = 0, total_b = 0;
    SS_TRY(hipMemGetInfo(&free_b, &total_b));
    long long limit = 0;                               // the matrix in half of the free device memory
    while ((unsigned long long)(limit + 1) * (unsigned long long)(limit + 1) * 8ull <= free_b / 2 && limit < 0x7FFFFFFEll) ++limit;
    out_stats16[0] = limit;
    if (n > limit) {
      char buf[160];
      snprintf(buf, sizeof buf, "%d samples: a distance matrix of at most %lld samples fits the free device memory", n, limit);
      return ss_fail(ctx, MIDAS_SNPS_ERR_OUT_OF_MEMORY, buf);
    }
  }
  const int steps = n - 3;
  SsBufs dev;
  SsEvents ev;
  for (int k = 0; k < 4; ++k) SS_TRY(hipEventCreate(&ev.e[k]));
  double *d_D = nullptr, *d_R = nullptr, *d_len = nullptr, *d_last_len = nullptr;
  uint8_t* d_active = nullptr;
  NjBest* d_part = nullptr;
  int *d_pair = nullptr, *d_join = nullptr, *d_last = nullptr, *d_err = nullptr;
  SS_TRY(dev.get(&d_D, nn * 8));
  SS_TRY(dev.get(&d_R, (size_t)n * 8));
  SS_TRY(dev.get(&d_len, (size_t)std::max(steps, 1) * 16));
  SS_TRY(dev.get(&d_last_len, 24));
  SS_TRY(dev.get(&d_active, (size_t)n));
  SS_TRY(dev.get(&d_part, (size_t)n * sizeof(NjBest)));
  SS_TRY(dev.get(&d_pair, 8));
  SS_TRY(dev.get(&d_join, (size_t)std::max(steps, 1) * 8));
  SS_TRY(dev.get(&d_last, 12));
  SS_TRY(dev.get(&d_err, 4));
  SS_TRY(hipEventRecord(ev.e[0], st));
  SS_TRY(hipMemcpyAsync(d_D, dist, nn * 8, hipMemcpyHostToDevice, st));
  SS_TRY(hipMemsetAsync(d_active, 1, (size_t)n, st));
  SS_TRY(hipMemsetAsync(d_err, 0, 4, st));
  SS_TRY(hipEventRecord(ev.e[1], st));
  for (int r = n; r > 3; --r) {
    const int step = n - r;
    hipLaunchKernelGGL(nj_sums_kernel, dim3(nblocks(n, kSumRows)), dim3(256), 0, st, d_D, d_active, n, d_R);
    hipLaunchKernelGGL(nj_row_min_kernel, dim3((unsigned)n), dim3(256), 0, st, d_D, d_active, d_R, n, r, d_part);
    hipLaunchKernelGGL(nj_choose_kernel, dim3(1), dim3(256), 0, st, d_D, d_R, d_part, n, r, step, d_pair, d_join, d_len, d_err);
    hipLaunchKernelGGL(nj_join_kernel, dim3(nblocks(n, 256)), dim3(256), 0, st, d_D, d_active, d_pair, n);
    SS_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(nj_last_kernel, dim3(1), dim3(64), 0, st, d_D, d_active, n, d_last, d_last_len, d_err);
  SS_TRY(hipGetLastError());
  SS_TRY(hipEventRecord(ev.e[2], st));
  int err = 0;
  if (steps > 0) {
    SS_TRY(hipMemcpyAsync(out_join, d_join, (size_t)steps * 8, hipMemcpyDeviceToHost, st));
    SS_TRY(hipMemcpyAsync(out_len, d_len, (size_t)steps * 16, hipMemcpyDeviceToHost, st));
  }
  SS_TRY(hipMemcpyAsync(out_last, d_last, 12, hipMemcpyDeviceToHost, st));
  SS_TRY(hipMemcpyAsync(out_last_len, d_last_len, 24, hipMemcpyDeviceToHost, st));
  SS_TRY(hipMemcpyAsync(&err, d_err, 4, hipMemcpyDeviceToHost, st));
  SS_TRY(hipEventRecord(ev.e[3], st));
  SS_TRY(hipStreamSynchronize(st));
  float ms[3] = {0.f, 0.f, 0.f};                       // upload, the steps, download
  for (int k = 0; k < 3; ++k) SS_TRY(hipEventElapsedTime(&ms[k], ev.e[k], ev.e[k + 1]));
  if (out_ms8) for (int k = 0; k < 3; ++k) out_ms8[k] = ms[k];
  out_stats16[1] = steps;
  out_stats16[2] = 4ll * steps + 1;
  if (err) return ss_fail(ctx, MIDAS_SNPS_ERR_INVALID_ARG, "a step found no pair to join: the Q values are not numbers");
  return MIDAS_SNPS_OK;
}
