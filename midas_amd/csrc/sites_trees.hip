// snp_trees.py on MI355X (midas_sites_consensus_pairs): the rows of snps_freq.txt / snps_depth.txt walked as midas_sites_scan
// walks them (RowGroups, sites_rows.h), the site kernel and the order of call_consensus.py (SiteStep, sites_call.h), then
//   planes   the consensus calls of a group's retained sites as two bit matrices [sample][64 retained sites a word], `called` and
//            `minor`, one wave a word (planes_by_sample_kernel over ConsensusCell, bit_planes.h)
//   pairs    both[i][j] += popcount(C_i & C_j), diff[i][j] += popcount(C_i & C_j & (M_i ^ M_j)), the tiling of the pair kernel
// This file is compiled with -ffp-contract=off (build.py), as every file that parses the cells and calls the sites.
#include "bit_planes.h"
#include "sites_call.h"

namespace midas {
namespace {

// retained site k of the group (rank among final_keep) -> its row
__global__ __launch_bounds__(256) void ss_keep_list_kernel(const uint8_t* final_keep, const uint32_t* rank, long long g, uint32_t* list) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r < g && final_keep[r]) list[rank[r]] = (uint32_t)r;
}

// both[i][j] += popcount(C_i & C_j), diff[i][j] += popcount(C_i & C_j & (M_i ^ M_j)) for i <= j: ss_pairs_kernel's tiling (a
// 64 x 64 tile of pairs a workgroup, a 4 x 4 part of it a thread, a run of words along blockIdx.y) over two planes.  Four strips
// are staged, 16 words at a time: the static LDS of ss_pairs_kernel's two strips of 32.
constexpr int kPlaneRun = kPairRun / 2;
__global__ __launch_bounds__(256) void ss_plane_pairs_kernel(const unsigned long long* called, const unsigned long long* minor,
                                                             long long wstride, long long n_words, long long run_words, int S,
                                                             int tiles_side, unsigned long long* both, unsigned long long* diff) {
  __shared__ unsigned long long ca[kPlaneRun][kPairPad], cb[kPlaneRun][kPairPad], ma[kPlaneRun][kPairPad], mb[kPlaneRun][kPairPad];
  const PairTile tile = pair_tile(blockIdx.x, tiles_side);
  const int ti = tile.ti, tj = tile.tj;
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const long long w0 = (long long)blockIdx.y * run_words, w1 = w0 + run_words < n_words ? w0 + run_words : n_words;
  uint32_t nb[4][4], nd[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) nb[i][j] = nd[i][j] = 0;
  for (long long k0 = w0; k0 < w1; k0 += kPlaneRun) {
#pragma unroll
    for (int it = 0; it < kPairTile * kPlaneRun / 256; ++it) {
      const int e = it * 256 + tid, s = e / kPlaneRun, k = e % kPlaneRun;
      const long long w = k0 + k;
      const int gi = ti * kPairTile + s, gj = tj * kPairTile + s;
      const bool on_i = gi < S && w < w1, on_j = gj < S && w < w1;
      ca[k][s] = on_i ? called[(long long)gi * wstride + w] : 0ull;
      ma[k][s] = on_i ? minor[(long long)gi * wstride + w] : 0ull;
      cb[k][s] = on_j ? called[(long long)gj * wstride + w] : 0ull;
      mb[k][s] = on_j ? minor[(long long)gj * wstride + w] : 0ull;
    }
    __syncthreads();
#pragma unroll 2
    for (int k = 0; k < kPlaneRun; ++k) {
      unsigned long long a[4], am[4], b[4], bm[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        a[i] = ca[k][ty + 16 * i]; am[i] = ma[k][ty + 16 * i];
        b[i] = cb[k][tx + 16 * i]; bm[i] = mb[k][tx + 16 * i];
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const unsigned long long c = a[i] & b[j];
          nb[i][j] += (uint32_t)__popcll(c);
          nd[i][j] += (uint32_t)__popcll(c & (am[i] ^ bm[j]));
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
        if (nb[i][j]) atomicAdd(&both[(long long)gi * S + gj], (unsigned long long)nb[i][j]);
        if (nd[i][j]) atomicAdd(&diff[(long long)gi * S + gj], (unsigned long long)nd[i][j]);
      }
    }
}

}  // namespace
}  // namespace midas

using namespace midas;

// midas_sites_scan's site decisions under MIDAS_SITES_SEQ, then the planes and the pair counts of every group
extern "C" int32_t midas_sites_consensus_pairs(midas_snps_ctx* ctx, const char* freq, int64_t freq_bytes, const char* depth, int64_t depth_bytes,
                                               int64_t n_sites_max, const uint8_t* site_mask, int32_t n_samples, const int32_t* sample_col,
                                               const double* mean_depth, const double* fparams5, const int64_t* iparams8, int64_t* out_both,
                                               int64_t* out_diff, int64_t* out_stats16, float* out_ms8) {
  if (!mean_depth || !fparams5 || !iparams8 || !out_both || !out_diff || (n_sites_max > 0 && !site_mask) || iparams8[4] < 0 ||
      iparams8[5] < 0 || iparams8[6] < 0)
    return MIDAS_SNPS_ERR_INVALID_ARG;
  const long long max_sites = iparams8[1];
  const int S = n_samples;
  std::vector<int32_t> col_slot;
  {
    const int32_t rc = sites_begin(ctx, freq, freq_bytes, depth, depth_bytes, n_sites_max, S, sample_col, out_stats16, out_ms8, &col_slot);
    if (rc != MIDAS_SNPS_OK) return rc;
  }
  const size_t n_acc = (size_t)S * (size_t)S;
  for (size_t k = 0; k < n_acc; ++k) out_both[k] = out_diff[k] = 0;
  SS_TRY(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  {
    // the two count matrices, and the distance matrix that follows them, in a quarter of the free device memory
    size_t free_b = 0, total_b = 0;
    SS_TRY(hipMemGetInfo(&free_b, &total_b));
    long long limit = 0;
    while ((unsigned long long)(limit + 1) * (unsigned long long)(limit + 1) * 16ull <= free_b / 4 && limit < 0x7FFFFFFEll) ++limit;
    out_stats16[13] = limit;
    if (S > limit) {
      char buf[160];
      snprintf(buf, sizeof buf, "%d samples: the pair matrices of at most %lld samples fit the free device memory", S, limit);
      return ss_fail(ctx, MIDAS_SNPS_ERR_OUT_OF_MEMORY, buf);
    }
  }
  if (n_sites_max == 0) return MIDAS_SNPS_OK;
  const long long per_row = (long long)S * (8 + 8 + 1 + 2 * (long long)sizeof(SideCell)) + 4 + 4 + 4 + 4 + 8 + 1 + 1 + 2 * ((S + 7) / 8);
  SsBufs dev;
  SsEvents ev;
  float ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};     // upload, index, parse, site, planes (order, list, planes), pairs, -, download
  RowGroups rg(ctx, dev, ev, ms, out_stats16);
  {
    // (max_sites 0: the reference converts the first row's cells and stops)
    const int32_t rc = rg.init(freq, freq_bytes, depth, depth_bytes, max_sites == 0 ? std::min<int64_t>(n_sites_max, 1) : n_sites_max, S,
                               col_slot, iparams8[4], iparams8[5], per_row);
    if (rc != MIDAS_SNPS_OK) return rc;
  }
  // (neither rounded nor weighted: nothing the reference raises on, so no error word)
  SiteStep site(ctx, rg, site_mask, iparams8[0], max_sites, fparams5, 0, 0, iparams8[2] & MIDAS_SITES_MASK_ONLY ? 1 : 0);
  {
    const int32_t rc = site.init(mean_depth, false);
    if (rc != MIDAS_SNPS_OK) return rc;
  }
  const long long G = rg.G, wstride = (G + 63) / 64;
  uint32_t* d_list = nullptr;
  unsigned long long *d_called = nullptr, *d_minor = nullptr, *d_both = nullptr, *d_diff = nullptr;
  SS_TRY(dev.get(&d_list, (size_t)G * 4));
  SS_TRY(dev.get(&d_called, (size_t)S * (size_t)wstride * 8));
  SS_TRY(dev.get(&d_minor, (size_t)S * (size_t)wstride * 8));
  SS_TRY(dev.get(&d_both, n_acc * 8));
  SS_TRY(dev.get(&d_diff, n_acc * 8));
  SS_TRY(hipMemsetAsync(d_both, 0, n_acc * 8, st));
  SS_TRY(hipMemsetAsync(d_diff, 0, n_acc * 8, st));
  const PairTiles tiles = pair_tiles(S, kPairTile);
  const long long pair_blocks = iparams8[6] > 0 ? iparams8[6] : 1024;      // workgroups the pair kernel aims at
  long long word_pairs = 0, max_runs = 0, max_steps = 0;
  bool stop = false;
  while (!stop) {
    long long g = 0;
    {
      const int32_t rc = rg.next(&g);
      if (rc != MIDAS_SNPS_OK) return rc;
    }
    if (g == 0) break;
    {
      const int32_t rc = site.run(g);
      if (rc != MIDAS_SNPS_OK) return rc;
    }
    hipLaunchKernelGGL(ss_keep_list_kernel, dim3(nblocks(g, 256)), dim3(256), 0, st, site.d_final, site.d_rank, g, d_list);
    SS_TRY(hipGetLastError());
    SS_TRY(hipStreamSynchronize(st));
    const long long kept_g = site.kept_g(), n_words = (kept_g + 63) / 64;
    if (kept_g > 0) {
      hipLaunchKernelGGL((planes_by_sample_kernel<2, ConsensusCell>), dim3((unsigned)n_words, (unsigned)((S + 3) / 4)), dim3(256), 0, st,
                         ConsensusCell{rg.d_fv, rg.d_dv, site.d_cell, d_list, G}, kept_g, S, wstride, d_called, d_minor);
      SS_TRY(hipGetLastError());
    }
    SS_TRY(hipEventRecord(ev.e[5], st));        // (again: the list and the planes count as the order's phase)
    if (kept_g > 0) {
      const PairRuns pr = pair_runs(n_words, tiles.n, pair_blocks, kPlaneRun);
      hipLaunchKernelGGL(ss_plane_pairs_kernel, dim3((unsigned)tiles.n, (unsigned)pr.runs), dim3(256), 0, st, d_called, d_minor, wstride,
                         n_words, pr.run_words, S, tiles.side, d_both, d_diff);
      SS_TRY(hipGetLastError());
      word_pairs += (long long)S * (S + 1) / 2 * n_words;
      max_runs = std::max(max_runs, pr.runs);
      max_steps = std::max(max_steps, pr.run_words / kPlaneRun);
    }
    SS_TRY(hipEventRecord(ev.e[6], st));
    SS_TRY(hipStreamSynchronize(st));
    SS_TRY(rg.lap(3, 4, 3));
    SS_TRY(rg.lap(4, 5, 4));
    SS_TRY(rg.lap(5, 6, 5));
    {
      const int32_t rc = site.check_rows();
      if (rc != MIDAS_SNPS_OK) return rc;
    }
    {
      const int32_t rc = site.advance(&stop);
      if (rc != MIDAS_SNPS_OK) return rc;
    }
  }
  SS_TRY(hipEventRecord(ev.e[0], st));
  SS_TRY(hipMemcpyAsync(out_both, d_both, n_acc * 8, hipMemcpyDeviceToHost, st));
  SS_TRY(hipMemcpyAsync(out_diff, d_diff, n_acc * 8, hipMemcpyDeviceToHost, st));
  SS_TRY(hipEventRecord(ev.e[1], st));
  SS_TRY(hipStreamSynchronize(st));
  SS_TRY(rg.lap(0, 1, 7));
  out_stats16[1] = site.kept;
  out_stats16[8] = word_pairs;
  out_stats16[11] = max_runs;
  out_stats16[12] = max_steps;
  sites_end(rg, out_ms8);
  return MIDAS_SNPS_OK;
}
