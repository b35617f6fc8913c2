// `merge_midas.py genes` on MI355X: the arithmetic of build_gene_matrices (/root/reference/midas/merge/genes.py:12-30) for
// all samples of a species at once.  Per (cluster, sample): the fp64 sums of copy number and depth over the sample's rows of
// the cluster IN TABLE ROW ORDER (the reference's `+=` into a defaultdict, which starts at 0.0), the integer sum of
// count_reads, whether the cluster appears in the sample's table at all, and presabs = copynum >= min_copy.  Output rows are
// the clusters that appear in sample 0's table (write_gene_matrices, genes.py:40), in cluster-index (= sorted id) order.
//
//   classes  samples whose tables list the same cluster sequence share one CSR (host: pointer or memcmp equality);
//   csr      once per class: stable radix sort of (cluster, row) pairs (device_sort.hip), so the rows of a cluster keep
//            their table order, and the first sorted position of every cluster;
//   rows     from sample 0's class: a flag per cluster that has rows, its exclusive scan, the compacted list;
//   groups   the samples of a class in runs of consecutive columns, at most `group` at a time (device memory bounded by
//            the caller's budget): their columns uploaded [sample][row], transposed to [row][sample], then
//   merge    one wave per output row (lanes = samples; more than 64 samples: 64 at a time), or, for fewer than 33 samples,
//            64 / S' rows a wave (S' = the samples rounded up to a power of two).  A row list is wave-uniform in the first
//            shape, every lane walks it in table order and adds exactly as the reference does; the loads of a table row
//            are contiguous across lanes.
// The outputs are [row][sample] row-major: what the matrix writer walks.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/midas_snps.h"
#include "ctx_internal.h"
#include "kernels.h"

namespace midas {
namespace {

__global__ __launch_bounds__(256) void gm_iota_kernel(uint32_t* v, long long n) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) v[i] = (uint32_t)i;
}

// begin[c] = first sorted position of cluster c (c in [0, n_clusters]; begin[n_clusters] = n)
__global__ __launch_bounds__(256) void gm_bounds_kernel(const uint32_t* key, long long n, long long n_clusters, long long* begin) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i > n) return;
  const long long prev = i == 0 ? -1 : (long long)key[i - 1];
  const long long cur = i == n ? n_clusters : (long long)key[i];
  for (long long g = prev + 1; g <= cur; ++g) begin[g] = i;
}

__global__ __launch_bounds__(256) void gm_flag_kernel(const long long* begin, long long n_clusters, uint32_t* flag) {
  const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
  if (c < n_clusters) flag[c] = begin[c + 1] > begin[c] ? 1u : 0u;
}

__global__ __launch_bounds__(256) void gm_compact_kernel(const long long* begin, const uint32_t* pos, long long n_clusters, uint32_t* rows) {
  const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
  if (c < n_clusters && begin[c + 1] > begin[c]) rows[pos[c]] = (uint32_t)c;
}

// [n_cols][n] -> [n][n_cols], 8-byte elements, 64 x 64 tiles through LDS
__global__ __launch_bounds__(256) void gm_transpose_kernel(const uint64_t* in, uint64_t* out, long long n, int n_cols) {
  __shared__ uint64_t tile[64][65];
  const long long r0 = (long long)blockIdx.x * 64;
  const int c0 = blockIdx.y * 64;
  for (int i = threadIdx.x; i < 64 * 64; i += 256) {
    const int cl = i >> 6, rl = i & 63;
    if (c0 + cl < n_cols && r0 + rl < n) tile[cl][rl] = in[(long long)(c0 + cl) * n + r0 + rl];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 64 * 64; i += 256) {
    const int rl = i >> 6, cl = i & 63;
    if (c0 + cl < n_cols && r0 + rl < n) out[(r0 + rl) * n_cols + c0 + cl] = tile[cl][rl];
  }
}

struct MergeKParams {
  const uint32_t* rows;        // [n_rows] output row -> cluster
  const long long* begin;      // [n_clusters + 1] the class's CSR
  const uint32_t* perm;        // [n] table rows, cluster-major, table order inside a cluster
  const double* copy;          // [n][n_cols]
  const double* depth;
  const int64_t* reads;
  double* out_copy;            // [n_rows][n_cols]
  double* out_depth;
  int64_t* out_reads;
  uint8_t* out_state;          // 0 absent from the table, 1 present below min_copy, 2 present at or above
  long long n_rows;
  int n_cols;
  double min_copy;
};

// one row a wave, lanes = samples (n_cols > 32): the row list is wave-uniform
__global__ __launch_bounds__(256) void gm_merge_wide_kernel(MergeKParams p) {
  const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= p.n_rows) return;
  const int lane = threadIdx.x & 63;
  const uint32_t c = __builtin_amdgcn_readfirstlane(p.rows[r]);
  const long long lo = p.begin[c], hi = p.begin[c + 1];
  const uint8_t present = hi > lo ? 1 : 0;
  for (int s = lane; s < p.n_cols; s += 64) {
    double cp = 0.0, dp = 0.0;
    int64_t rd = 0;
    for (long long k = lo; k < hi; ++k) {
      const long long row = (long long)__builtin_amdgcn_readfirstlane(p.perm[k]);
      const long long at = row * p.n_cols + s;
      cp += p.copy[at];
      dp += p.depth[at];
      rd += p.reads[at];
    }
    const long long o = r * p.n_cols + s;
    p.out_copy[o] = cp;
    p.out_depth[o] = dp;
    p.out_reads[o] = rd;
    p.out_state[o] = present ? (cp >= p.min_copy ? 2 : 1) : 0;
  }
}

// 64 / sp rows a wave, sp lanes each (sp = n_cols rounded up to a power of two, <= 32)
__global__ __launch_bounds__(256) void gm_merge_narrow_kernel(MergeKParams p, int sp_log2) {
  const int lane = threadIdx.x & 63, sp = 1 << sp_log2;
  const long long r = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * (64 >> sp_log2) + (lane >> sp_log2);
  const int s = lane & (sp - 1);
  if (r >= p.n_rows || s >= p.n_cols) return;
  const uint32_t c = p.rows[r];
  const long long lo = p.begin[c], hi = p.begin[c + 1];
  double cp = 0.0, dp = 0.0;
  int64_t rd = 0;
  for (long long k = lo; k < hi; ++k) {
    const long long at = (long long)p.perm[k] * p.n_cols + s;
    cp += p.copy[at];
    dp += p.depth[at];
    rd += p.reads[at];
  }
  const long long o = r * p.n_cols + s;
  p.out_copy[o] = cp;
  p.out_depth[o] = dp;
  p.out_reads[o] = rd;
  p.out_state[o] = hi > lo ? (cp >= p.min_copy ? 2 : 1) : 0;
}

int32_t gm_fail(midas_snps_ctx* ctx, int32_t st, const char* msg) {
  ctx->set_error(msg);
  return st;
}

#define GM_TRY(call)                                                                                             \
  do {                                                                                                           \
    hipError_t e__ = (call);                                                                                     \
    if (e__ != hipSuccess) {                                                                                     \
      char buf__[384];                                                                                           \
      snprintf(buf__, sizeof buf__, "%s: %s", #call, hipGetErrorString(e__));                                    \
      (void)hipGetLastError();                                                                                   \
      return gm_fail(ctx, e__ == hipErrorOutOfMemory ? MIDAS_SNPS_ERR_OUT_OF_MEMORY : MIDAS_SNPS_ERR_HIP, buf__); \
    }                                                                                                            \
  } while (0)

struct GmBufs {        // device buffers of one call, freed when it returns
  std::vector<void*> ptrs;
  ~GmBufs() { for (void* q : ptrs) (void)hipFree(q); }
  template <class T> hipError_t get(T** out, size_t bytes) {
    void* q = nullptr;
    const hipError_t e = hipMalloc(&q, bytes ? bytes : 16);
    if (e == hipSuccess) ptrs.push_back(q);
    *out = static_cast<T*>(q);
    return e;
  }
};

unsigned blocks_of(long long n, long long per) { return (unsigned)((n + per - 1) / per); }

}  // namespace
}  // namespace midas

using namespace midas;

extern "C" int32_t midas_genes_merge(midas_snps_ctx* ctx, int32_t n_samples, const int64_t* n_rows, const uint32_t* const* cluster,
                                     const double* const* copy, const double* const* depth, const int64_t* const* reads,
                                     int64_t n_clusters, double min_copy, int32_t group_samples, int64_t out_capacity,
                                     int64_t* out_n_rows, uint32_t* out_row_cluster, double* out_copy, double* out_depth,
                                     int64_t* out_reads, uint8_t* out_state, float* out_kernel_ms) {
  if (!ctx || n_samples < 1 || !n_rows || !cluster || !copy || !depth || !reads || n_clusters < 0 || n_clusters > 0xFFFFFFFFll ||
      out_capacity < 0 || !out_n_rows || (out_capacity > 0 && (!out_row_cluster || !out_copy || !out_depth || !out_reads || !out_state)))
    return MIDAS_SNPS_ERR_INVALID_ARG;
  ctx->clear_error();
  ctx->err_read = -1;
  *out_n_rows = 0;
  if (out_kernel_ms) *out_kernel_ms = 0.f;
  const int S = n_samples;
  // ---- host: classes of equal cluster sequences, and the checks that keep every device index in bounds --------------------
  std::vector<int> cls((size_t)S, -1), rep;
  for (int s = 0; s < S; ++s) {
    if (n_rows[s] < 0 || n_rows[s] > 0x7FFFFFFFll || (n_rows[s] > 0 && (!cluster[s] || !copy[s] || !depth[s] || !reads[s])))
      return MIDAS_SNPS_ERR_INVALID_ARG;
    for (size_t k = 0; k < rep.size() && cls[(size_t)s] < 0; ++k) {
      const int r = rep[k];
      if (n_rows[r] == n_rows[s] && (n_rows[s] == 0 || cluster[r] == cluster[s] || memcmp(cluster[r], cluster[s], (size_t)n_rows[s] * 4) == 0))
        cls[(size_t)s] = (int)k;
    }
    if (cls[(size_t)s] < 0) {
      for (int64_t i = 0; i < n_rows[s]; ++i)
        if ((int64_t)cluster[s][i] >= n_clusters) {
          ctx->err_read = i;
          char buf[160];
          snprintf(buf, sizeof buf, "sample %d, row %lld: cluster index %u is outside the %lld clusters", s, (long long)i, cluster[s][i],
                   (long long)n_clusters);
          return gm_fail(ctx, MIDAS_SNPS_ERR_BAD_LAYOUT, buf);
        }
      cls[(size_t)s] = (int)rep.size();
      rep.push_back(s);
    }
  }
  if (n_clusters == 0) return MIDAS_SNPS_OK;      // (no cluster: every table is empty, no row)
  GM_TRY(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  GmBufs dev;
  const size_t C = (size_t)n_clusters;
  int64_t n_max = 1;
  for (int s = 0; s < S; ++s) n_max = std::max<int64_t>(n_max, n_rows[s]);
  const size_t nm = (size_t)n_max;
  uint32_t *d_key = nullptr, *d_key_b = nullptr, *d_val = nullptr, *d_val_b = nullptr, *d_scratch = nullptr, *d_flag = nullptr,
           *d_rows = nullptr;
  long long* d_begin = nullptr;
  GM_TRY(dev.get(&d_key, nm * 4));
  GM_TRY(dev.get(&d_key_b, nm * 4));
  GM_TRY(dev.get(&d_val, nm * 4));
  GM_TRY(dev.get(&d_val_b, nm * 4));
  GM_TRY(dev.get(&d_scratch, std::max(sort_scratch_words((long long)nm), scan_scratch_words((long long)C)) * 4));
  GM_TRY(dev.get(&d_begin, (C + 1) * 8));
  GM_TRY(dev.get(&d_flag, C * 4));
  GM_TRY(dev.get(&d_rows, C * 4));
  int key_bits = 1;
  while (key_bits < 32 && ((int64_t)1 << key_bits) < n_clusters) ++key_bits;
  struct EvGuard {
    hipEvent_t a = nullptr, b = nullptr;
    ~EvGuard() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
  } evg;
  GM_TRY(hipEventCreate(&evg.a));
  GM_TRY(hipEventCreate(&evg.b));
  uint32_t* perm = nullptr;
  float kernel_ms = 0.f;       // device time of the kernels (events around them; the copies in between are not counted)
  // the CSR of class k: d_begin + perm (one of d_val / d_val_b)
  auto build_csr = [&](int k) -> int32_t {
    const int s = rep[(size_t)k];
    const long long n = (long long)n_rows[s];
    if (n == 0) {
      GM_TRY(hipMemsetAsync(d_begin, 0, (C + 1) * 8, st));
      perm = d_val;
      return MIDAS_SNPS_OK;
    }
    GM_TRY(hipMemcpyAsync(d_key, cluster[s], (size_t)n * 4, hipMemcpyHostToDevice, st));
    GM_TRY(hipEventRecord(evg.a, st));
    hipLaunchKernelGGL(gm_iota_kernel, dim3(blocks_of(n, 256)), dim3(256), 0, st, d_val, n);
    GM_TRY(hipGetLastError());
    uint32_t* key_sorted = d_key;
    perm = d_val;
    GM_TRY(launch_sort_pairs_u32(d_key, d_val, d_key_b, d_val_b, n, key_bits, d_scratch, st, &key_sorted, &perm));
    hipLaunchKernelGGL(gm_bounds_kernel, dim3(blocks_of(n + 1, 256)), dim3(256), 0, st, key_sorted, n, (long long)n_clusters, d_begin);
    GM_TRY(hipGetLastError());
    GM_TRY(hipEventRecord(evg.b, st));
    GM_TRY(hipEventSynchronize(evg.b));
    float ms = 0.f;
    GM_TRY(hipEventElapsedTime(&ms, evg.a, evg.b));
    kernel_ms += ms;
    return MIDAS_SNPS_OK;
  };
  int32_t rc = build_csr(0);
  if (rc != MIDAS_SNPS_OK) return rc;
  // output rows: the clusters sample 0's table mentions
  hipLaunchKernelGGL(gm_flag_kernel, dim3(blocks_of((long long)C, 256)), dim3(256), 0, st, d_begin, (long long)C, d_flag);
  GM_TRY(hipGetLastError());
  uint32_t last_flag = 0, last_pos = 0;
  GM_TRY(hipMemcpyAsync(&last_flag, d_flag + C - 1, 4, hipMemcpyDeviceToHost, st));
  GM_TRY(launch_scan_u32(d_flag, d_flag, (long long)C, d_scratch, st));
  GM_TRY(hipMemcpyAsync(&last_pos, d_flag + C - 1, 4, hipMemcpyDeviceToHost, st));
  hipLaunchKernelGGL(gm_compact_kernel, dim3(blocks_of((long long)C, 256)), dim3(256), 0, st, d_begin, d_flag, (long long)C, d_rows);
  GM_TRY(hipGetLastError());
  GM_TRY(hipStreamSynchronize(st));
  const long long R = (long long)last_pos + last_flag;
  if (R > out_capacity) {
    char buf[128];
    snprintf(buf, sizeof buf, "%lld output rows do not fit out_capacity = %lld", R, (long long)out_capacity);
    return gm_fail(ctx, MIDAS_SNPS_ERR_INVALID_ARG, buf);
  }
  *out_n_rows = R;
  if (R == 0) return MIDAS_SNPS_OK;
  GM_TRY(hipMemcpyAsync(out_row_cluster, d_rows, (size_t)R * 4, hipMemcpyDeviceToHost, st));
  // ---- column groups: runs of consecutive samples of one class, at most G samples --------------------------------------------
  long long G = group_samples;
  if (G <= 0) {
    size_t free_b = 0, total_b = 0;
    GM_TRY(hipMemGetInfo(&free_b, &total_b));
    const size_t per = (size_t)n_max * 48 + (size_t)R * 25;       // a sample's columns, their transpose, its output cells
    G = (long long)std::max<size_t>(1, free_b / 4 / per);
  }
  G = std::min<long long>(G, S);
  double *d_cin = nullptr, *d_copy = nullptr, *d_depth = nullptr, *o_copy = nullptr, *o_depth = nullptr;
  int64_t* d_reads = nullptr;
  int64_t* o_reads = nullptr;
  uint8_t* o_state = nullptr;
  const size_t cells_in = nm * (size_t)G, cells_out = (size_t)R * (size_t)G;
  GM_TRY(dev.get(&d_cin, cells_in * 8));
  GM_TRY(dev.get(&d_copy, cells_in * 8));
  GM_TRY(dev.get(&d_depth, cells_in * 8));
  GM_TRY(dev.get(&d_reads, cells_in * 8));
  GM_TRY(dev.get(&o_copy, cells_out * 8));
  GM_TRY(dev.get(&o_depth, cells_out * 8));
  GM_TRY(dev.get(&o_reads, cells_out * 8));
  GM_TRY(dev.get(&o_state, cells_out));
  std::vector<uint8_t> stage;          // a group's outputs on their way into the [R][S] host matrices (groups narrower than S)
  for (int k = 0; k < (int)rep.size(); ++k) {
    if (k > 0) {
      rc = build_csr(k);
      if (rc != MIDAS_SNPS_OK) return rc;
    }
    const long long n = (long long)n_rows[rep[(size_t)k]];
    for (int s0 = 0; s0 < S;) {
      if (cls[(size_t)s0] != k) { ++s0; continue; }
      int s1 = s0 + 1;
      while (s1 < S && s1 - s0 < G && cls[(size_t)s1] == k) ++s1;
      const int g = s1 - s0;
      // upload [sample][row] and transpose to [row][sample], column kind by column kind
      const void* const* srcs[3] = {(const void* const*)copy, (const void* const*)depth, (const void* const*)reads};
      void* dsts[3] = {d_copy, d_depth, d_reads};
      float ms = 0.f;
      for (int kind = 0; kind < 3 && n > 0; ++kind) {
        for (int j = 0; j < g; ++j)
          GM_TRY(hipMemcpyAsync(d_cin + (size_t)j * (size_t)n, srcs[kind][s0 + j], (size_t)n * 8, hipMemcpyHostToDevice, st));
        GM_TRY(hipEventRecord(evg.a, st));
        hipLaunchKernelGGL(gm_transpose_kernel, dim3(blocks_of(n, 64), blocks_of(g, 64)), dim3(256), 0, st, (const uint64_t*)d_cin,
                           (uint64_t*)dsts[kind], n, g);
        GM_TRY(hipGetLastError());
        GM_TRY(hipEventRecord(evg.b, st));
        GM_TRY(hipEventSynchronize(evg.b));      // (the staging buffer d_cin is written again by the next kind's uploads)
        float t = 0.f;
        GM_TRY(hipEventElapsedTime(&t, evg.a, evg.b));
        ms += t;
      }
      GM_TRY(hipEventRecord(evg.a, st));
      MergeKParams p;
      p.rows = d_rows; p.begin = d_begin; p.perm = perm; p.copy = d_copy; p.depth = d_depth; p.reads = d_reads;
      p.out_copy = o_copy; p.out_depth = o_depth; p.out_reads = o_reads; p.out_state = o_state;
      p.n_rows = R; p.n_cols = g; p.min_copy = min_copy;
      if (g > 32) {
        hipLaunchKernelGGL(gm_merge_wide_kernel, dim3(blocks_of(R, 4)), dim3(256), 0, st, p);
      } else {
        int lg = 0;
        while ((1 << lg) < g) ++lg;
        const long long per_block = 4ll * (64 >> lg);
        hipLaunchKernelGGL(gm_merge_narrow_kernel, dim3(blocks_of(R, per_block)), dim3(256), 0, st, p, lg);
      }
      GM_TRY(hipGetLastError());
      GM_TRY(hipEventRecord(evg.b, st));
      if (g == S) {
        GM_TRY(hipMemcpyAsync(out_copy, o_copy, (size_t)R * S * 8, hipMemcpyDeviceToHost, st));
        GM_TRY(hipMemcpyAsync(out_depth, o_depth, (size_t)R * S * 8, hipMemcpyDeviceToHost, st));
        GM_TRY(hipMemcpyAsync(out_reads, o_reads, (size_t)R * S * 8, hipMemcpyDeviceToHost, st));
        GM_TRY(hipMemcpyAsync(out_state, o_state, (size_t)R * S, hipMemcpyDeviceToHost, st));
        GM_TRY(hipStreamSynchronize(st));
      } else {
        stage.resize((size_t)R * (size_t)g * 25);
        uint8_t* h = stage.data();
        GM_TRY(hipMemcpyAsync(h, o_copy, (size_t)R * g * 8, hipMemcpyDeviceToHost, st));
        GM_TRY(hipMemcpyAsync(h + (size_t)R * g * 8, o_depth, (size_t)R * g * 8, hipMemcpyDeviceToHost, st));
        GM_TRY(hipMemcpyAsync(h + (size_t)R * g * 16, o_reads, (size_t)R * g * 8, hipMemcpyDeviceToHost, st));
        GM_TRY(hipMemcpyAsync(h + (size_t)R * g * 24, o_state, (size_t)R * g, hipMemcpyDeviceToHost, st));
        GM_TRY(hipStreamSynchronize(st));
        for (long long r = 0; r < R; ++r) {
          const size_t src = (size_t)r * g, dst = (size_t)r * S + s0;
          memcpy(out_copy + dst, h + src * 8, (size_t)g * 8);
          memcpy(out_depth + dst, h + (size_t)R * g * 8 + src * 8, (size_t)g * 8);
          memcpy(out_reads + dst, h + (size_t)R * g * 16 + src * 8, (size_t)g * 8);
          memcpy(out_state + dst, h + (size_t)R * g * 24 + src, (size_t)g);
        }
      }
      float t = 0.f;
      GM_TRY(hipEventElapsedTime(&t, evg.a, evg.b));
      kernel_ms += ms + t;
      s0 = s1;
    }
  }
  if (out_kernel_ms) *out_kernel_ms = kernel_ms;
  return MIDAS_SNPS_OK;
}
