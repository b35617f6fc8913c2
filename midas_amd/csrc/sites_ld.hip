// snp_ld.py on MI355X (midas_sites_ld): linkage disequilibrium between pairs of retained sites, by distance.
// The rows of snps_freq.txt / snps_depth.txt are walked as midas_sites_consensus_pairs walks them (RowGroups, sites_rows.h; SiteStep,
// sites_call.h); then
//   planes   the consensus calls of a group's retained sites, appended SITE-major to two resident bit matrices [retained site]
//            [64 samples a word], `called` and `minor`, with the site's key and gene beside them: the window of an anchor never
//            sees a group border.  A workgroup takes 64 retained sites x 64 samples: a wave ballots a sample's 64 sites (the cell
//            reads run along the sites, as the cells lie), the 64 x 64 bit block is turned in LDS (planes_by_row_kernel over
//            ConsensusCell, bit_planes.h)
//   ld       one wave an anchor; lanes take 64 consecutive partners a step, four popcount sums over the words each; the terms go
//            through LDS, and one lane a quantity adds them in lane order.  The bin of a partner never falls along the walk, so a
//            lane carries ONE running sum and stores it when the bin changes: p[anchor][bin] without bins in LDS
//   fold     one lane a (bin, quantity) chain over the chunk's anchors in order, from the carried total
// This file is compiled with -ffp-contract=off (build.py), as every file that parses the cells and calls the sites.
#include "bit_planes.h"
#include "sites_call.h"

namespace midas {
namespace {

constexpr int kLdQ = 5;                 // a (anchor, bin) holds r2, d2, het (double) and window, pairs (int64), 8 bytes each
constexpr int kLdMaxBins = 4096;

// retained site k of the group (rank among final_keep) -> its row; its key and gene go behind those of the groups before
__global__ __launch_bounds__(256) void ld_keep_list_kernel(const uint8_t* final_keep, const uint32_t* rank, long long g, const long long* gkey,
                                                           const int32_t* ggene, long long room, uint32_t* list, long long* key,
                                                           int32_t* gene) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r >= g || !final_keep[r]) return;
  const uint32_t k = rank[r];
  if ((long long)k >= room) return;             // (never: the host has counted the rows that can be retained)
  list[k] = (uint32_t)r;
  key[k] = gkey[r];
  gene[k] = ggene ? ggene[r] : 0;
}

struct LdP {
  const unsigned long long *called, *minor;   // [M][W]
  const long long* key;                        // [M], strictly ascending
  const int32_t* gene;                         // [M]
  long long M, a0, a1;                         // the retained sites; the chunk's anchors
  int W, n_bins, same_gene;
  long long max_dist, bin_width, min_samples;
  unsigned long long* p;                       // [a1 - a0][n_bins][kLdQ], zeroed
};

// One wave (a workgroup of its own, so that __syncthreads orders its LDS traffic) an anchor.
__global__ __launch_bounds__(64) void ld_pairs_kernel(LdP q) {
  __shared__ int code[64];                     // -1: no pair; else bin << 1 | informative
  __shared__ double term[3][64];
  const long long a = q.a0 + blockIdx.x;
  if (a >= q.a1) return;
  const int lane = threadIdx.x, W = q.W;
  const long long key_a = q.key[a];
  const int gene_a = q.gene[a];
  const unsigned long long *ca = q.called + a * W, *ma = q.minor + a * W;
  unsigned long long* out = q.p + (long long)blockIdx.x * q.n_bins * kLdQ;
  // lanes 0..4 each carry one quantity of the bin the walk is in
  int cur = -1;
  double acc = 0.0;
  long long cnt = 0;
  for (long long b0 = a + 1; b0 < q.M; b0 += 64) {
    const long long b = b0 + lane;
    bool in_range = false, pair = false, inf = false;
    int bin = 0;
    double r2 = 0.0, d2 = 0.0, het = 0.0;
    if (b < q.M) {
      const long long dist = q.key[b] - key_a;
      in_range = dist >= 1 && dist <= q.max_dist;
      pair = in_range && (!q.same_gene || (gene_a >= 0 && q.gene[b] == gene_a));
      if (pair) {
        bin = (int)((dist - 1) / q.bin_width);
        const unsigned long long *cb = q.called + b * W, *mb = q.minor + b * W;
        int n = 0, na = 0, nb = 0, nab = 0;
        for (int w = 0; w < W; ++w) {
          const unsigned long long c = ca[w] & cb[w], xa = c & ma[w], xb = c & mb[w];
          n += __popcll(c);
          na += __popcll(xa);
          nb += __popcll(xb);
          nab += __popcll(xa & xb);
        }
        inf = n >= q.min_samples && 0 < na && na < n && 0 < nb && nb < n;
        if (inf) {
          const long long Dn = (long long)n * nab - (long long)na * nb;
          const long long ha = (long long)na * (n - na), hb = (long long)nb * (n - nb);
          const double num = __dmul_rn((double)Dn, (double)Dn);
          const double den = __dmul_rn((double)ha, (double)hb);
          r2 = __ddiv_rn(num, den);
          const double n2 = (double)((long long)n * n);
          const double n4 = __dmul_rn(n2, n2);
          d2 = __ddiv_rn(num, n4);
          het = __ddiv_rn(den, n4);
        }
      }
    }
    code[lane] = pair ? (bin << 1) | (inf ? 1 : 0) : -1;
    term[0][lane] = r2;
    term[1][lane] = d2;
    term[2][lane] = het;
    __syncthreads();
    if (lane < kLdQ) {
      for (int l = 0; l < 64; ++l) {
        const int c = code[l];
        if (c < 0) continue;
        const int bl = c >> 1;
        if (bl != cur) {
          if (cur >= 0) out[(long long)cur * kLdQ + lane] = lane < 3 ? (unsigned long long)__double_as_longlong(acc) : (unsigned long long)cnt;
          cur = bl;
          acc = 0.0;
          cnt = 0;
        }
        if (lane < 3) {
          if (c & 1) acc += term[lane][l];
        } else if (lane == 3 || (c & 1)) {
          ++cnt;
        }
      }
    }
    __syncthreads();
    if (__ballot(!in_range) != 0ull) break;     // a lane past the window (or past the last site): every later one is too
  }
  if (lane < kLdQ && cur >= 0) out[(long long)cur * kLdQ + lane] = lane < 3 ? (unsigned long long)__double_as_longlong(acc) : (unsigned long long)cnt;
}

// total[bin][quantity] += p[anchor][bin][quantity] over the chunk's anchors in order: one lane a chain.  The few waves this
// takes wait on memory, not on the adds: kFoldAhead loads are in flight ahead of the adds, which stay one after another.
constexpr int kFoldAhead = 32;
__global__ __launch_bounds__(64) void ld_fold_kernel(const unsigned long long* p, long long n_anchors, int n_chains, unsigned long long* total) {
  const int t = blockIdx.x * 64 + threadIdx.x;
  if (t >= n_chains) return;
  const bool is_f64 = t % kLdQ < 3;
  double acc = is_f64 ? __longlong_as_double((long long)total[t]) : 0.0;
  unsigned long long cnt = total[t];
  long long a = 0;
  for (; a + kFoldAhead <= n_anchors; a += kFoldAhead) {
    unsigned long long v[kFoldAhead];
#pragma unroll
    for (int i = 0; i < kFoldAhead; ++i) v[i] = p[(a + i) * n_chains + t];
#pragma unroll
    for (int i = 0; i < kFoldAhead; ++i) {
      if (is_f64) acc += __longlong_as_double((long long)v[i]);
      else cnt += v[i];
    }
  }
  for (; a < n_anchors; ++a) {
    const unsigned long long v = p[a * n_chains + t];
    if (is_f64) acc += __longlong_as_double((long long)v);
    else cnt += v;
  }
  total[t] = is_f64 ? (unsigned long long)__double_as_longlong(acc) : cnt;
}

}  // namespace
}  // namespace midas

using namespace midas;

// midas_sites_scan's site decisions under MIDAS_SITES_SEQ, the resident site-major planes, then the pairs of sites by anchor chunk
extern "C" int32_t midas_sites_ld(midas_snps_ctx* ctx, const char* freq, int64_t freq_bytes, const char* depth, int64_t depth_bytes,
                                  int64_t n_sites_max, const uint8_t* site_mask, int32_t n_samples, const int32_t* sample_col,
                                  const double* mean_depth, const double* fparams5, const int64_t* iparams8, const int64_t* site_key,
                                  const int32_t* site_gene, int64_t max_dist, int64_t bin_width, int64_t* out_window, int64_t* out_pairs,
                                  double* out_sum_r2, double* out_sum_d2, double* out_sum_het, int64_t* out_stats16, float* out_ms8) {
  if (!mean_depth || !fparams5 || !iparams8 || !out_window || !out_pairs || !out_sum_r2 || !out_sum_d2 || !out_sum_het ||
      (n_sites_max > 0 && (!site_mask || !site_key)) || iparams8[4] < 0 || iparams8[5] < 0 || iparams8[6] < 0 || max_dist < 1 ||
      max_dist >= (1ll << 39) || bin_width < 1)
    return MIDAS_SNPS_ERR_INVALID_ARG;
  const long long n_bins_ll = (max_dist + bin_width - 1) / bin_width;
  const int same_gene = iparams8[2] & MIDAS_SITES_LD_SAME_GENE ? 1 : 0;
  if (n_bins_ll > kLdMaxBins || (same_gene && n_sites_max > 0 && !site_gene)) return MIDAS_SNPS_ERR_INVALID_ARG;
  const int n_bins = (int)n_bins_ll, n_chains = n_bins * kLdQ;
  const long long max_sites = iparams8[1], min_samples = iparams8[3];
  const int S = n_samples;
  std::vector<int32_t> col_slot;
  {
    const int32_t rc = sites_begin(ctx, freq, freq_bytes, depth, depth_bytes, n_sites_max, S, sample_col, out_stats16, out_ms8, &col_slot);
    if (rc != MIDAS_SNPS_OK) return rc;
  }
  for (int k = 0; k < n_bins; ++k) {
    out_window[k] = out_pairs[k] = 0;
    out_sum_r2[k] = out_sum_d2[k] = out_sum_het[k] = 0.0;
  }
  // the rows that can be retained: their keys ascend strictly, and their number bounds the planes
  long long m_cap = 0;
  {
    long long last = -1;
    for (int64_t r = 0; r < n_sites_max; ++r) {
      if (!site_mask[r]) continue;
      if (site_key[r] < 0 || (last >= 0 && site_key[r] <= last)) {
        char buf[160];
        snprintf(buf, sizeof buf, "data row %lld: the site keys of the rows in the mask do not ascend strictly", (long long)r);
        out_stats16[5] = r;
        return ss_fail(ctx, MIDAS_SNPS_ERR_INVALID_ARG, buf);
      }
      last = site_key[r];
      ++m_cap;
    }
    if (max_sites >= 0) m_cap = std::min(m_cap, max_sites);
  }
  const int W = (S + 63) / 64;
  SS_TRY(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  {
    // the two planes, the keys and the genes of the retained sites in a quarter of the free device memory
    size_t free_b = 0, total_b = 0;
    SS_TRY(hipMemGetInfo(&free_b, &total_b));
    const long long limit = (long long)((free_b / 4) / ((size_t)W * 16 + 12));
    out_stats16[13] = limit;
    if (m_cap > limit) {
      char buf[200];
      snprintf(buf, sizeof buf, "%lld sites may be retained: the planes of at most %lld sites of %d samples fit the free device memory", m_cap,
               limit, S);
      return ss_fail(ctx, MIDAS_SNPS_ERR_OUT_OF_MEMORY, buf);
    }
  }
  if (n_sites_max == 0) return MIDAS_SNPS_OK;
  const long long per_row = (long long)S * (8 + 8 + 1 + 2 * (long long)sizeof(SideCell)) + 4 + 4 + 4 + 4 + 8 + 1 + 1 + 8 + 4;
  SsBufs dev;
  SsEvents ev;
  float ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};     // upload, index, parse, site, planes (order, list, planes), ld, fold, download
  RowGroups rg(ctx, dev, ev, ms, out_stats16);
  {
    const int32_t rc = rg.init(freq, freq_bytes, depth, depth_bytes, max_sites == 0 ? std::min<int64_t>(n_sites_max, 1) : n_sites_max, S,
                               col_slot, iparams8[4], iparams8[5], per_row);
    if (rc != MIDAS_SNPS_OK) return rc;
  }
  SiteStep site(ctx, rg, site_mask, iparams8[0], max_sites, fparams5, 0, 0, iparams8[2] & MIDAS_SITES_MASK_ONLY ? 1 : 0);
  {
    const int32_t rc = site.init(mean_depth, false);
    if (rc != MIDAS_SNPS_OK) return rc;
  }
  const long long G = rg.G;
  const size_t cap = (size_t)std::max<long long>(m_cap, 1);
  uint32_t* d_list = nullptr;
  long long *d_gkey = nullptr, *d_key = nullptr;
  int32_t *d_ggene = nullptr, *d_gene = nullptr;
  unsigned long long *d_called = nullptr, *d_minor = nullptr, *d_total = nullptr, *d_p = nullptr;
  SS_TRY(dev.get(&d_list, (size_t)G * 4));
  SS_TRY(dev.get(&d_gkey, (size_t)G * 8));
  if (site_gene) SS_TRY(dev.get(&d_ggene, (size_t)G * 4));
  SS_TRY(dev.get(&d_key, cap * 8));
  SS_TRY(dev.get(&d_gene, cap * 4));
  SS_TRY(dev.get(&d_called, cap * (size_t)W * 8));
  SS_TRY(dev.get(&d_minor, cap * (size_t)W * 8));
  SS_TRY(dev.get(&d_total, (size_t)n_chains * 8));
  SS_TRY(hipMemsetAsync(d_total, 0, (size_t)n_chains * 8, st));
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
    const long long m0 = site.kept;           // (kept never passes m_cap: a retained row has its mask set, and max_sites bounds both)
    SS_TRY(hipMemcpyAsync(d_gkey, site_key + rg.base, (size_t)g * 8, hipMemcpyHostToDevice, st));
    if (site_gene) SS_TRY(hipMemcpyAsync(d_ggene, site_gene + rg.base, (size_t)g * 4, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(ld_keep_list_kernel, dim3(nblocks(g, 256)), dim3(256), 0, st, site.d_final, site.d_rank, g, d_gkey, d_ggene, m_cap - m0,
                       d_list, d_key + m0, d_gene + m0);
    SS_TRY(hipGetLastError());
    SS_TRY(hipStreamSynchronize(st));
    const long long kept_g = site.kept_g();
    if (m0 + kept_g > m_cap) return ss_fail(ctx, MIDAS_SNPS_ERR_INVALID_ARG, "more sites retained than the mask holds");
    if (kept_g > 0) {
      hipLaunchKernelGGL((planes_by_row_kernel<2, ConsensusCell>), dim3(nblocks(kept_g, 64), (unsigned)W), dim3(256), 0, st,
                         ConsensusCell{rg.d_fv, rg.d_dv, site.d_cell, d_list, G}, kept_g, S, W, d_called + m0 * W, d_minor + m0 * W);
      SS_TRY(hipGetLastError());
    }
    SS_TRY(hipEventRecord(ev.e[5], st));        // (the list and the planes count as the order's phase)
    SS_TRY(hipStreamSynchronize(st));
    SS_TRY(rg.lap(3, 4, 3));
    SS_TRY(rg.lap(4, 5, 4));
    {
      const int32_t rc = site.check_rows();
      if (rc != MIDAS_SNPS_OK) return rc;
    }
    {
      const int32_t rc = site.advance(&stop);
      if (rc != MIDAS_SNPS_OK) return rc;
    }
  }
  // ---- the pairs of sites, a chunk of anchors at a time ---------------------------------------------------------------------
  const long long M = site.kept;
  long long chunk = iparams8[6];
  if (chunk == 0) chunk = std::min<long long>(1 << 20, std::max<long long>(256, (256ll << 20) / ((long long)n_chains * 8)));
  chunk = std::max<long long>(1, std::min(chunk, std::max<long long>(M, 1)));
  SS_TRY(dev.get(&d_p, (size_t)chunk * (size_t)n_chains * 8));
  long long chunks = 0;
  for (long long a0 = 0; a0 < M; a0 += chunk, ++chunks) {
    const long long a1 = std::min(M, a0 + chunk);
    LdP q;
    q.called = d_called; q.minor = d_minor; q.key = d_key; q.gene = d_gene; q.M = M; q.a0 = a0; q.a1 = a1; q.W = W; q.n_bins = n_bins;
    q.same_gene = same_gene; q.max_dist = max_dist; q.bin_width = bin_width; q.min_samples = min_samples; q.p = d_p;
    SS_TRY(hipEventRecord(ev.e[0], st));
    SS_TRY(hipMemsetAsync(d_p, 0, (size_t)(a1 - a0) * (size_t)n_chains * 8, st));
    hipLaunchKernelGGL(ld_pairs_kernel, dim3((unsigned)(a1 - a0)), dim3(64), 0, st, q);
    SS_TRY(hipGetLastError());
    SS_TRY(hipEventRecord(ev.e[1], st));
    hipLaunchKernelGGL(ld_fold_kernel, dim3(nblocks(n_chains, 64)), dim3(64), 0, st, d_p, a1 - a0, n_chains, d_total);
    SS_TRY(hipGetLastError());
    SS_TRY(hipEventRecord(ev.e[6], st));
    SS_TRY(hipStreamSynchronize(st));
    SS_TRY(rg.lap(0, 1, 5));
    SS_TRY(rg.lap(1, 6, 6));
  }
  std::vector<unsigned long long> total((size_t)n_chains);
  SS_TRY(hipEventRecord(ev.e[0], st));
  SS_TRY(hipMemcpyAsync(total.data(), d_total, (size_t)n_chains * 8, hipMemcpyDeviceToHost, st));
  SS_TRY(hipEventRecord(ev.e[1], st));
  SS_TRY(hipStreamSynchronize(st));
  SS_TRY(rg.lap(0, 1, 7));
  long long visited = 0;
  for (int k = 0; k < n_bins; ++k) {
    const unsigned long long* t = &total[(size_t)k * kLdQ];
    memcpy(&out_sum_r2[k], &t[0], 8);
    memcpy(&out_sum_d2[k], &t[1], 8);
    memcpy(&out_sum_het[k], &t[2], 8);
    out_window[k] = (int64_t)t[3];
    out_pairs[k] = (int64_t)t[4];
    visited += out_window[k];
  }
  out_stats16[1] = M;
  out_stats16[8] = visited;
  out_stats16[11] = chunks;
  out_stats16[12] = chunk;
  sites_end(rg, out_ms8);
  return MIDAS_SNPS_OK;
}
