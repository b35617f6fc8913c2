// snp_pairs.py on MI355X (midas_sites_pair_diversity): for every two of the selected samples what `snp_diversity.py --sample_type
// pooled-samples` gives with exactly those two selected, and beside it the sums of the within-sample and between-sample pi over
// the sites both samples are kept at.  The rows are walked as midas_sites_scan walks them (RowGroups, sites_rows.h); the site
// kernel runs with mask_only (SiteStep, sites_call.h) and leaves every (site, sample) cell flagged as flag_samples flags it; then
//   pairs    prevalence, pooled frequency, --site_prev, --site_maf and --max_sites depend on which two samples are pooled, so
//            they are decided per (pair, site) here.  A lane owns whole pairs, a P x P patch of them in registers, and walks the
//            group's rows front to back: the site axis is never split, every sum is the sequential one.  A workgroup owns a
//            16P x 16P tile of pairs and stages the cells of its row-samples and column-samples through LDS, kSpRun rows at a
//            time; the next run's loads are issued before the current run is folded.  P = 1 by default, P = 4 on request.
// The accumulators live in [S][S] device arrays, loaded at a group's start and stored at its end: no bit of the result depends on
// the row groups or on the tile.  This file is compiled with -ffp-contract=off (build.py): every sum and product rounds once.
#include "sites_call.h"

namespace midas {
namespace {

constexpr int kSpRun = 16;                     // rows of every sample staged at a time
constexpr int kSpRoomMax = 0x7FFFFFFF;         // a pair without --max_sites: more room than a group has rows

struct PairDivP {
  const double* fv;            // [S][stride]
  const long long* dv;         // [S][stride]
  const uint8_t* cell;         // [S][stride] bit 0: the sample is kept at the site
  const uint8_t* row_keep;     // [g] what the info table and the options decide
  long long g, stride;
  int S, tiles_side, round_freq;
  int need_count;              // --site_prev: the fewest kept cells of the two (0: no test; 3: none passes)
  long long max_sites;         // per pair; < 0: all
  double site_maf, snp_maf;
  double *pi, *w1, *w2, *x;    // [S][S], the upper triangle
  long long *sites, *snps, *shared;
};

// Tile (ti, tj), ti <= tj, of T = 16 P samples a side; thread (ty, tx) owns the pairs (ti T + ty + 16 i, tj T + tx + 16 j).
// W: --weight_by_depth, the depths are staged too.
template <int P, bool W>
__global__ __launch_bounds__(256) void sp_pairs_kernel(PairDivP p) {
  constexpr int T = 16 * P, PAD = T + 1;
  __shared__ double sf[2][kSpRun][PAD];
  __shared__ long long sd[W ? 2 : 1][W ? kSpRun : 1][W ? PAD : 1];
  __shared__ uint8_t sk[2][kSpRun][T];
  const PairTile tile = pair_tile(blockIdx.x, p.tiles_side);
  const int ti = tile.ti, tj = tile.tj;
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int base_s[2] = {ti * T, tj * T};

  double pi[P][P], w1[P][P], w2[P][P], xs[P][P];
  int room[P][P];
  uint32_t snps[P][P], shared[P][P];
#pragma unroll
  for (int i = 0; i < P; ++i)
#pragma unroll
    for (int j = 0; j < P; ++j) {
      const int gi = base_s[0] + ty + 16 * i, gj = base_s[1] + tx + 16 * j;
      pi[i][j] = w1[i][j] = w2[i][j] = xs[i][j] = 0.0;
      room[i][j] = 0;
      snps[i][j] = shared[i][j] = 0;
      if (gi < gj && gj < p.S) {
        const long long at = (long long)gi * p.S + gj;
        pi[i][j] = p.pi[at]; w1[i][j] = p.w1[at]; w2[i][j] = p.w2[at]; xs[i][j] = p.x[at];
        long long r = kSpRoomMax;
        if (p.max_sites >= 0) {
          r = p.max_sites - p.sites[at];
          r = r < 0 ? 0 : r > kSpRoomMax ? kSpRoomMax : r;
        }
        room[i][j] = (int)r;
      }
    }

  // what this thread stages of a run: element e = it * 256 + tid is row e % kSpRun of tile sample e / kSpRun, for both sides
  double nf[2][P];
  long long nd[2][P];
  uint8_t nk[2][P];
  auto load_run = [&](long long r0) {
#pragma unroll
    for (int side = 0; side < 2; ++side)
#pragma unroll
      for (int it = 0; it < P; ++it) {
        const int e = it * 256 + tid, k = e % kSpRun, s = e / kSpRun;
        const int gs = base_s[side] + s;
        const long long r = r0 + k;
        const bool on = gs < p.S && r < p.g;
        const long long at = on ? (long long)gs * p.stride + r : 0;
        const double f = p.fv[at];
        const uint8_t c = p.cell[at], m = p.row_keep[on ? r : 0];
        nf[side][it] = on ? f : 0.0;
        nk[side][it] = on ? (uint8_t)((c & 1) | (m ? 2 : 0)) : (uint8_t)0;
        if (W) nd[side][it] = on ? p.dv[at] : 0;
      }
  };

  if (p.g > 0) load_run(0);
  for (long long r0 = 0; r0 < p.g; r0 += kSpRun) {
    __syncthreads();                             // (the run before is folded)
#pragma unroll
    for (int side = 0; side < 2; ++side)
#pragma unroll
      for (int it = 0; it < P; ++it) {
        const int e = it * 256 + tid, k = e % kSpRun, s = e / kSpRun;
        const double f = nf[side][it];
        sf[side][k][s] = p.round_freq ? rint(f) + 0.0 : f;      // (float(round(f)) is never -0.0)
        sk[side][k][s] = nk[side][it];
        if (W) sd[side][k][s] = nd[side][it];
      }
    __syncthreads();
    if (r0 + kSpRun < p.g) load_run(r0 + kSpRun);              // in flight while this run is folded
#pragma unroll(P == 1 ? 2 : 1)
    for (int k = 0; k < kSpRun; ++k) {
      // per sample of the patch: f, 1 - f, (2 f)(1 - f), and the start of the pooled sum (0.0 + f, or 0.0 + d f weighted)
      double a[P], oa[P], ha[P], a0[P], b[P], ob[P], hb[P], b0[P], wb[P];
      long long da[P], db[P];
      int ka[P], kb[P];
#pragma unroll
      for (int i = 0; i < P; ++i) {
        a[i] = sf[0][k][ty + 16 * i];
        ka[i] = sk[0][k][ty + 16 * i];
        oa[i] = 1.0 - a[i];
        ha[i] = (2.0 * a[i]) * oa[i];
        if (W) {
          da[i] = sd[0][k][ty + 16 * i];
          a0[i] = 0.0 + (double)da[i] * a[i];
        } else {
          da[i] = 0;
          a0[i] = 0.0 + a[i];
        }
        b[i] = sf[1][k][tx + 16 * i];
        kb[i] = sk[1][k][tx + 16 * i];
        ob[i] = 1.0 - b[i];
        hb[i] = (2.0 * b[i]) * ob[i];
        if (W) {
          db[i] = sd[1][k][tx + 16 * i];
          wb[i] = (double)db[i] * b[i];
        } else {
          db[i] = 0;
          wb[i] = b[i];
        }
        b0[i] = 0.0 + wb[i];
      }
#pragma unroll
      for (int i = 0; i < P; ++i)
#pragma unroll
        for (int j = 0; j < P; ++j) {
          const bool ki = (ka[i] & 1) != 0, kj = (kb[j] & 1) != 0;
          const int count = (ki ? 1 : 0) + (kj ? 1 : 0);
          // site_pooled over the two cells, i before j: the sum starts from 0.0 and takes the kept values in order
          const double sum = ki ? (kj ? a0[i] + wb[j] : a0[i]) : (kj ? b0[j] : 0.0);
          double pooled;
          if (W) {
            const long long dsum = (ki ? da[i] : 0) + (kj ? db[j] : 0);
            pooled = count ? __ddiv_rn(sum, (double)dsum) : 0.0;
          } else {
            pooled = count == 2 ? sum * 0.5 : sum;      // sum / count: x * 0.5 and x / 2.0 round the same real number
          }
          bool keep = (ka[i] & kb[j] & 2) != 0 && count >= p.need_count && room[i][j] > 0;
          if (p.site_maf != 0.0 && pooled < p.site_maf) keep = false;
          room[i][j] -= keep ? 1 : 0;
          const double op = 1.0 - pooled;
          const double term = (2.0 * pooled) * op;
          double m = pooled;                            // min(p, 1 - p) as Python's min
          if (op < m) m = op;
          // (a sum that starts from +0.0 is never -0.0, so adding +0.0 leaves every bit as it is)
          pi[i][j] += keep ? term : 0.0;
          snps[i][j] += keep && m >= p.snp_maf ? 1u : 0u;
          const bool both = keep && count == 2;
          shared[i][j] += both ? 1u : 0u;
          w1[i][j] += both ? ha[i] : 0.0;
          w2[i][j] += both ? hb[j] : 0.0;
          const double between = (a[i] * ob[j]) + (b[j] * oa[i]);
          xs[i][j] += both ? between : 0.0;
        }
    }
  }

#pragma unroll
  for (int i = 0; i < P; ++i)
#pragma unroll
    for (int j = 0; j < P; ++j) {
      const int gi = base_s[0] + ty + 16 * i, gj = base_s[1] + tx + 16 * j;
      if (gi < gj && gj < p.S) {
        const long long at = (long long)gi * p.S + gj;
        p.pi[at] = pi[i][j]; p.w1[at] = w1[i][j]; p.w2[at] = w2[i][j]; p.x[at] = xs[i][j];
        const long long before = p.sites[at];
        long long r = kSpRoomMax;
        if (p.max_sites >= 0) {
          r = p.max_sites - before;
          r = r < 0 ? 0 : r > kSpRoomMax ? kSpRoomMax : r;
        }
        p.sites[at] = before + (r - room[i][j]);
        p.snps[at] += snps[i][j];
        p.shared[at] += shared[i][j];
      }
    }
}

template <int P>
void sp_launch(const PairDivP& q, bool weight, long long n_tiles, hipStream_t st) {
  if (weight) hipLaunchKernelGGL((sp_pairs_kernel<P, true>), dim3((unsigned)n_tiles), dim3(256), 0, st, q);
  else hipLaunchKernelGGL((sp_pairs_kernel<P, false>), dim3((unsigned)n_tiles), dim3(256), 0, st, q);
}

}  // namespace
}  // namespace midas

using namespace midas;

extern "C" int32_t midas_sites_pair_diversity(midas_snps_ctx* ctx, const char* freq, int64_t freq_bytes, const char* depth, int64_t depth_bytes,
                                              int64_t n_sites_max, const uint8_t* site_mask, int32_t n_samples, const int32_t* sample_col,
                                              const double* mean_depth, const double* fparams5, const int64_t* iparams8, int64_t* out_sites,
                                              int64_t* out_snps, int64_t* out_shared, double* out_pi, double* out_w1, double* out_w2,
                                              double* out_x, int64_t* out_stats16, float* out_ms8) {
  if (!mean_depth || !fparams5 || !iparams8 || !out_sites || !out_snps || !out_shared || !out_pi || !out_w1 || !out_w2 || !out_x ||
      (n_sites_max > 0 && !site_mask) || n_samples < 2 || iparams8[4] < 0 || iparams8[5] < 0 || iparams8[6] < 0 || iparams8[6] > 2)
    return MIDAS_SNPS_ERR_INVALID_ARG;
  const long long site_depth = iparams8[0], max_sites = iparams8[1] < 0 ? -1 : iparams8[1], flags = iparams8[2];
  const int weight = flags & MIDAS_SITES_WEIGHT ? 1 : 0, round_freq = flags & MIDAS_SITES_ROUND ? 1 : 0;
  // (a kept cell has at least site_depth reads: from 1 on, the weighted pool of a pair never divides by 0)
  if (weight && site_depth < 1) return MIDAS_SNPS_ERR_INVALID_ARG;
  const int S = n_samples;
  std::vector<int32_t> col_slot;
  {
    const int32_t rc = sites_begin(ctx, freq, freq_bytes, depth, depth_bytes, n_sites_max, S, sample_col, out_stats16, out_ms8, &col_slot);
    if (rc != MIDAS_SNPS_OK) return rc;
  }
  SS_TRY(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  {
    // the seven accumulator matrices in a quarter of the free device memory
    size_t free_b = 0, total_b = 0;
    SS_TRY(hipMemGetInfo(&free_b, &total_b));
    long long limit = 0;
    while ((unsigned long long)(limit + 1) * (unsigned long long)(limit + 1) * 56ull <= free_b / 4 && limit < 0x7FFFFFFEll) ++limit;
    out_stats16[13] = limit;
    if (S > limit) {
      char buf[160];
      snprintf(buf, sizeof buf, "%d samples: the pair matrices of at most %lld samples fit the free device memory", S, limit);
      return ss_fail(ctx, MIDAS_SNPS_ERR_OUT_OF_MEMORY, buf);
    }
  }
  const size_t n_acc = (size_t)S * (size_t)S;
  for (size_t k = 0; k < n_acc; ++k) {
    out_sites[k] = out_snps[k] = out_shared[k] = 0;
    out_pi[k] = out_w1[k] = out_w2[k] = out_x[k] = 0.0;
  }
  if (n_sites_max == 0) return MIDAS_SNPS_OK;
  SsBufs dev;
  SsEvents ev;
  float ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};     // upload, index, parse, site, order, pairs, -, download
  void* d_acc[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  for (void*& a : d_acc) {
    SS_TRY(dev.get((char**)&a, n_acc * 8));
    SS_TRY(hipMemsetAsync(a, 0, n_acc * 8, st));
  }
  const long long per_row = (long long)S * (8 + 8 + 1 + 2 * (long long)sizeof(SideCell)) + 4 + 4 + 4 + 4 + 8 + 1 + 1;
  RowGroups rg(ctx, dev, ev, ms, out_stats16);
  {
    const int32_t rc = rg.init(freq, freq_bytes, depth, depth_bytes, n_sites_max, S, col_slot, iparams8[4], iparams8[5], per_row);
    if (rc != MIDAS_SNPS_OK) return rc;
  }
  // mask_only, no --max_sites: the site kernel flags the cells and reports a frequency --consensus cannot round; what depends
  // on the pair is the pair kernel's
  SiteStep site(ctx, rg, site_mask, site_depth, -1, fparams5, 0, round_freq, 1);
  {
    const int32_t rc = site.init(mean_depth, round_freq != 0);
    if (rc != MIDAS_SNPS_OK) return rc;
  }
  // one pair a lane (tiles of 16 x 16) unless the caller forces the 4 x 4 patch: on an MI355X the first form was the faster one at
  // every sample count measured, 50 to 1 500 (profiles/snp_pairs.txt) -- the fold is bound by its instructions, not by the loads
  const int patch = iparams8[6] == 2 ? 4 : 1;
  const PairTiles tiles = pair_tiles(S, 16 * patch);
  if (tiles.n > 0x7FFFFFFFll) return ss_fail(ctx, MIDAS_SNPS_ERR_UNSUPPORTED, "more pair tiles than a grid holds");
  PairDivP q;
  q.fv = rg.d_fv; q.dv = rg.d_dv; q.cell = site.d_cell; q.row_keep = site.d_final; q.stride = rg.G; q.S = S; q.tiles_side = tiles.side;
  q.round_freq = round_freq; q.max_sites = max_sites; q.site_maf = fparams5[3]; q.snp_maf = fparams5[4];
  {
    // GenomicSite.filter's prevalence test, count / 2 against max(1e-6, site_prev), once for the three counts there are
    const double site_prev = fparams5[2], thr = 1e-6 > site_prev ? 1e-6 : site_prev;
    q.need_count = 0;
    if (site_prev != 0.0) {
      q.need_count = 3;
      for (int c = 2; c >= 0; --c)
        if (!((double)c / 2.0 < thr)) q.need_count = c;
    }
  }
  q.sites = (long long*)d_acc[0]; q.snps = (long long*)d_acc[1]; q.shared = (long long*)d_acc[2];
  q.pi = (double*)d_acc[3]; q.w1 = (double*)d_acc[4]; q.w2 = (double*)d_acc[5]; q.x = (double*)d_acc[6];
  const long long n_pairs = (long long)S * (S - 1) / 2;
  long long pair_sites = 0;
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
    q.g = g;
    if (patch == 1) sp_launch<1>(q, weight != 0, tiles.n, st);
    else sp_launch<4>(q, weight != 0, tiles.n, st);
    SS_TRY(hipGetLastError());
    pair_sites += n_pairs * g;
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
  void* out[7] = {out_sites, out_snps, out_shared, out_pi, out_w1, out_w2, out_x};
  SS_TRY(hipEventRecord(ev.e[0], st));
  for (int k = 0; k < 7; ++k) SS_TRY(hipMemcpyAsync(out[k], d_acc[k], n_acc * 8, hipMemcpyDeviceToHost, st));
  SS_TRY(hipEventRecord(ev.e[1], st));
  SS_TRY(hipStreamSynchronize(st));
  SS_TRY(rg.lap(0, 1, 7));
  out_stats16[1] = site.kept;
  out_stats16[8] = pair_sites;
  out_stats16[11] = patch;
  out_stats16[12] = tiles.n;
  sites_end(rg, out_ms8);
  return MIDAS_SNPS_OK;
}
