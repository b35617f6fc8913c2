// snp_diversity.py --rand_reads N [--replace_reads] over a row group, between the site kernel and the ordered sums
// (sites_scan.hip): GenomicSite.resample_reads and the compute_pooled_maf behind it, for every retained site whose pooled
// frequency is above 0.  Every selected sample of such a site gets depth N, kept or not; a cell with 0 < f < 1 gets
// f = k / N, where count_minor = round(f * N) (half to even) and k is count_minor without replacement, or the number of
// the cell's N draws below count_minor with replacement.  The draws are numpy's: np.random.choice(list of N, N) is
// randint(0, N, N), which takes MT19937 words, masks them and keeps those <= N - 1 (draw_plan.h).  N is the same for every
// cell, so the accepted words are ONE subsequence of the raw stream, and the c-th cell that draws -- sites in file order,
// samples in their order -- owns accepted words [c * N, (c + 1) * N).
//   eligible  one thread a row: the site is resampled (redo), how many of its cells draw (cnt).  The cells lie [S][stride], so
//             the (row, sample) order of the drawing cells is a per-row count plus the library's scan over the rows -- no
//             transposed flag array; a second pass a row then lists count_minor of its drawing cells from the row's offset on
//   generate  mt19937_stream.hip, a launch of raw words at a time, until the accepted words cover what the rows at hand need
//   compact   exclusive scan of the launch's accept flags (device_sort.hip), the masked values scattered behind those there.
//             What a group leaves over -- accepted words beyond its need, and with them the raw words behind -- the next
//             group starts with: results and the final state depend neither on group_rows nor on the launch size
//   hits      one thread a WORD, a wave over 64 consecutive accepted words: ballot of (word < count_minor of its cell), one
//             atomicAdd a (wave, cell) of the population count of the cell's lanes.  No thread strides by N
//   write     one thread a row: depth N for all S cells of a resampled site, f = k / N for the drawing ones, in place
//   pool      one thread a row: the pooled frequency of a resampled site again, by the site kernel's own site_pooled()
// With N = 1 or without replacement nothing is drawn and k = count_minor.  Internal linkage; -ffp-contract=off (build.py):
// f * N rounds once, as the interpreter rounds it.
#pragma once
#include <array>
#include <deque>
#include <memory>

#include "draw_plan.h"
#include "sites_call.h"

namespace midas {
namespace {

struct ResampleP {
  double* fv;                  // [S][stride]
  long long* dv;
  const uint8_t* cell;
  const uint8_t* final_keep;   // [g]
  double* pooled;              // [g]
  long long g, stride;
  int S, round_freq, weight;
  long long N;
  uint32_t* cnt;               // [g] cells of the row that draw
  const uint32_t* off;         // [g] exclusive scan of cnt
  uint8_t* redo;               // [g] the site is resampled
  uint32_t* cm;                // [cells that draw] count_minor, in (row, sample) order
  const uint32_t* k;           // [cells that draw] minor reads after resampling
  unsigned long long* n_redo;
};

__device__ __forceinline__ bool rs_draws(double f, int round_freq) {
  const double f2 = round_freq ? rint(f) + 0.0 : f;
  return f2 > 0.0 && f2 < 1.0;
}

__global__ __launch_bounds__(256) void rs_eligible_kernel(ResampleP p) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  bool redo = false;
  uint32_t n = 0;
  if (r < p.g) {
    redo = p.final_keep[r] && p.pooled[r] > 0.0;
    if (redo)
      for (int s = 0; s < p.S; ++s) n += rs_draws(p.fv[(long long)s * p.stride + r], p.round_freq) ? 1u : 0u;
    p.cnt[r] = n;
    p.redo[r] = redo ? 1 : 0;
  }
  const unsigned long long any = __ballot(redo);
  if ((threadIdx.x & 63) == 0 && any) atomicAdd(p.n_redo, (unsigned long long)__popcll((long long)any));
}

__global__ __launch_bounds__(256) void rs_cells_kernel(ResampleP p) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r >= p.g || !p.redo[r]) return;
  uint32_t j = p.off[r];
  for (int s = 0; s < p.S; ++s) {
    const double f = p.fv[(long long)s * p.stride + r];
    if (rs_draws(f, p.round_freq)) p.cm[j++] = (uint32_t)rint(f * (double)p.N);     // (a frequency that draws is not rounded: f2 == f)
  }
}

// words [0, n_words) of `acc` belong to cells e0, e0 + 1, ..., N each
__global__ __launch_bounds__(256) void rs_hits_kernel(const uint32_t* acc, const uint32_t* cm, uint32_t* k, uint32_t e0, unsigned long long N,
                                                      unsigned long long n_words) {
  const unsigned long long w = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
  const unsigned lane = threadIdx.x & 63;
  const unsigned long long w0 = w - lane;
  const bool in = w < n_words;
  const unsigned long long e = in ? w / N : 0;
  const bool hit = in && acc[w] < cm[e0 + e];
  const unsigned long long hits = __ballot(hit);
  if (!in) return;
  const unsigned long long lo = e * N > w0 ? e * N : w0;
  if (w != lo) return;                                   // the first lane of the cell's run inside the wave adds for the run
  unsigned long long hi = (e + 1) * N;
  if (hi > w0 + 64) hi = w0 + 64;
  if (hi > n_words) hi = n_words;
  const unsigned a = (unsigned)(lo - w0), b = (unsigned)(hi - w0);       // lanes [a, b), 0 <= a < b <= 64
  const unsigned long long run = (b == 64 ? ~0ull : (1ull << b) - 1) & ~((1ull << a) - 1);
  const unsigned c = (unsigned)__popcll((long long)(hits & run));
  if (c) atomicAdd(&k[e0 + e], c);
}

__global__ __launch_bounds__(256) void rs_write_kernel(ResampleP p) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r >= p.g || !p.redo[r]) return;
  uint32_t j = p.off[r];
  for (int s = 0; s < p.S; ++s) {
    const long long at = (long long)s * p.stride + r;
    if (rs_draws(p.fv[at], p.round_freq)) p.fv[at] = __ddiv_rn((double)p.k[j++], (double)p.N);
    p.dv[at] = p.N;
  }
}

__global__ __launch_bounds__(256) void rs_pool_kernel(ResampleP p) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r >= p.g || !p.redo[r]) return;
  long long count = 0;
  for (int s = 0; s < p.S; ++s) count += p.cell[(long long)s * p.stride + r] & 1;
  bool zero_depth = false;                              // (never: every depth is N >= 1)
  p.pooled[r] = site_pooled(p.fv + r, p.dv + r, p.cell + r, p.stride, p.S, count, p.weight, p.round_freq, &zero_depth);
}

// The host side: the buffers, the draw ledger (draw_plan.h) and the stream from launch to launch.  run() goes between
// SiteStep::run() and the sums of a group; collect() after the caller has synchronised; finish() once, behind the last group.
struct ResampleStep {
  static constexpr long long kChunkDefault = 1ll << 22, kBatchWords = 1ll << 26, kBatchMax = 1ll << 30;
  midas_snps_ctx* ctx;
  RowGroups& rg;
  SiteStep& site;
  long long N;
  bool draws;                    // with replacement and N > 1: the only case that takes words from the stream
  long long chunk_cap = 0, batch_words = 0, cap = 0;
  ResampleP rp;
  uint32_t *d_cnt = nullptr, *d_off = nullptr, *d_cm = nullptr, *d_k = nullptr, *d_state = nullptr, *d_flag = nullptr, *d_place = nullptr,
           *d_masked = nullptr, *d_acc = nullptr, *d_acc_at = nullptr, *d_sums = nullptr;
  uint8_t* d_redo = nullptr;
  unsigned long long* d_n_redo = nullptr;
  hipEvent_t e[8] = {};          // 0-1 eligible; 2-3-4 generate, compact; 5-6-7 (hits,) write, pool
  std::vector<uint32_t> off_h;
  DrawLedger led;
  std::deque<std::array<uint32_t, 625>> starts;      // the generator state each chunk of led.chunks started from
  std::array<uint32_t, 625> first{};
  long long head = 0, tail = 0;  // the unused accepted words are d_acc[head, tail)
  uint32_t last_at = 0;          // the last used accepted word's index among the raw words of its chunk
  long long resampled = 0, cells_drew = 0;
  double ms[5] = {0, 0, 0, 0, 0};        // eligible, generate, compact, resample (hits + write), re-pool
  bool pending = false;

  ResampleStep(midas_snps_ctx* c, RowGroups& r, SiteStep& s, long long n, int replace) : ctx(c), rg(r), site(s), N(n), draws(replace && n > 1) {}
  ~ResampleStep() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }

  // device bytes a row of the group takes here
  static long long per_row(int S) { return (long long)S * 8 + 9; }

  int32_t init(long long chunk_in, const uint32_t* key624, int32_t pos) {
    hipStream_t st = rg.st;
    const size_t G = (size_t)rg.G;
    for (auto& x : e) SS_TRY(hipEventCreate(&x));
    SS_TRY(rg.dev.get(&d_cnt, G * 4));
    SS_TRY(rg.dev.get(&d_off, G * 4));
    SS_TRY(rg.dev.get(&d_redo, G));
    SS_TRY(rg.dev.get(&d_cm, rg.cells * 4));
    SS_TRY(rg.dev.get(&d_n_redo, 8));
    SS_TRY(hipMemsetAsync(d_n_redo, 0, 8, st));
    for (int i = 0; i < 624; ++i) first[(size_t)i] = key624[i];
    first[624] = (uint32_t)pos;
    if (draws) {
      if ((long long)rg.S * N > kBatchMax) return ss_fail(ctx, MIDAS_SNPS_ERR_UNSUPPORTED, "samples x rand_reads beyond 2^30 draws a site");
      chunk_cap = chunk_in > 0 ? std::max<long long>(chunk_in, 64) : kChunkDefault;
      // (a group never needs more than cells x N words at once; a site's cells are never split)
      const unsigned __int128 most = (unsigned __int128)rg.cells * (unsigned __int128)N;
      batch_words = std::max<long long>((long long)rg.S * N, most < (unsigned __int128)kBatchWords ? (long long)most : kBatchWords);
      cap = batch_words + 2 * chunk_cap;
      SS_TRY(rg.dev.get(&d_k, rg.cells * 4));
      SS_TRY(rg.dev.get(&d_state, 625 * 4));
      SS_TRY(rg.dev.get(&d_flag, (size_t)chunk_cap * 4));
      SS_TRY(rg.dev.get(&d_place, (size_t)chunk_cap * 4));
      SS_TRY(rg.dev.get(&d_masked, (size_t)chunk_cap * 4));
      SS_TRY(rg.dev.get(&d_sums, scan_scratch_words(chunk_cap) * 4));
      SS_TRY(rg.dev.get(&d_acc, (size_t)cap * 4));
      SS_TRY(rg.dev.get(&d_acc_at, (size_t)cap * 4));
      SS_TRY(hipMemcpyAsync(d_state, first.data(), 625 * 4, hipMemcpyHostToDevice, st));
    }
    rp.fv = rg.d_fv; rp.dv = rg.d_dv; rp.cell = site.d_cell; rp.final_keep = site.d_final; rp.pooled = site.d_pooled; rp.stride = rg.G;
    rp.S = rg.S; rp.round_freq = site.sp.round_freq; rp.weight = site.sp.weight; rp.N = N; rp.cnt = d_cnt; rp.off = d_off; rp.redo = d_redo;
    rp.cm = d_cm; rp.k = draws ? d_k : d_cm; rp.n_redo = d_n_redo;
    return MIDAS_SNPS_OK;
  }

  int32_t lap(int a, int b, int slot) {
    float t = 0.f;
    SS_TRY(hipEventElapsedTime(&t, e[a], e[b]));
    ms[slot] += t;
    return MIDAS_SNPS_OK;
  }

  // accepted words until `need` of them are unused; the stream is waited for after every launch (its yield decides the next)
  int32_t top_up(long long need) {
    hipStream_t st = rg.st;
    const uint32_t bound = (uint32_t)(N - 1), mask = draw_mask(N);
    while (led.available() < need) {
      const long long n = draw_request(need - led.available(), N, chunk_cap);
      if (tail + n > cap) return ss_fail(ctx, MIDAS_SNPS_ERR_HIP, "resampling: the accepted words outgrew their buffer");
      starts.emplace_back();
      SS_TRY(hipMemcpyAsync(starts.back().data(), d_state, 625 * 4, hipMemcpyDeviceToHost, st));
      SS_TRY(hipEventRecord(e[2], st));
      SS_TRY(launch_mt_stream(d_state, n, nullptr, d_flag, d_masked, mask, bound, st));
      SS_TRY(hipEventRecord(e[3], st));
      SS_TRY(launch_scan_u32(d_flag, d_place, n, d_sums, st));
      SS_TRY(launch_mt_scatter(d_flag, d_place, d_masked, n, d_acc + tail, d_acc_at + tail, st));
      SS_TRY(hipEventRecord(e[4], st));
      uint32_t last_place = 0, last_flag = 0;
      SS_TRY(hipMemcpyAsync(&last_place, d_place + n - 1, 4, hipMemcpyDeviceToHost, st));
      SS_TRY(hipMemcpyAsync(&last_flag, d_flag + n - 1, 4, hipMemcpyDeviceToHost, st));
      SS_TRY(hipStreamSynchronize(st));
      const long long got = (long long)last_place + last_flag;
      led.add(n, got);
      tail += got;
      { const int32_t rc = lap(2, 3, 1); if (rc != MIDAS_SNPS_OK) return rc; }
      { const int32_t rc = lap(3, 4, 2); if (rc != MIDAS_SNPS_OK) return rc; }
    }
    return MIDAS_SNPS_OK;
  }

  // the group of g rows whose site kernel and order are enqueued
  int32_t run(long long g) {
    hipStream_t st = rg.st;
    rp.g = g;
    const unsigned nb = nblocks(g, 256);
    uint32_t last_off = 0, last_cnt = 0;
    SS_TRY(hipEventRecord(e[0], st));
    hipLaunchKernelGGL(rs_eligible_kernel, dim3(nb), dim3(256), 0, st, rp);
    SS_TRY(hipGetLastError());
    SS_TRY(launch_scan_u32(d_cnt, d_off, g, rg.d_scratch, st));
    hipLaunchKernelGGL(rs_cells_kernel, dim3(nb), dim3(256), 0, st, rp);
    SS_TRY(hipGetLastError());
    SS_TRY(hipEventRecord(e[1], st));
    SS_TRY(hipMemcpyAsync(&last_off, d_off + g - 1, 4, hipMemcpyDeviceToHost, st));
    SS_TRY(hipMemcpyAsync(&last_cnt, d_cnt + g - 1, 4, hipMemcpyDeviceToHost, st));
    if (draws) {
      off_h.resize((size_t)g + 1);
      SS_TRY(hipMemcpyAsync(off_h.data(), d_off, (size_t)g * 4, hipMemcpyDeviceToHost, st));
    }
    SS_TRY(hipStreamSynchronize(st));
    { const int32_t rc = lap(0, 1, 0); if (rc != MIDAS_SNPS_OK) return rc; }
    const long long E = (long long)last_off + last_cnt;
    cells_drew += E;
    if (draws && E > 0) {
      off_h[(size_t)g] = (uint32_t)E;
      SS_TRY(hipMemsetAsync(d_k, 0, (size_t)E * 4, st));
      // rows [r0, r1) at a time: as many whole sites as the accepted buffer holds the words of
      long long r0 = 0;
      while (r0 < g) {
        const long long e0 = off_h[(size_t)r0];
        const long long fit = e0 + batch_words / N;
        long long r1 = (long long)(std::upper_bound(off_h.begin() + r0, off_h.end(), (uint32_t)std::min<long long>(fit, 0xFFFFFFFFll)) - off_h.begin()) - 1;
        r1 = std::min(std::max(r1, r0 + 1), g);
        const long long need = ((long long)off_h[(size_t)r1] - e0) * N;
        if (need > 0) {
          const long long live = tail - head;
          if (head > 0 && head >= live) {          // the words left over move to the front (they never overlap there)
            if (live > 0) {
              SS_TRY(hipMemcpyAsync(d_acc, d_acc + head, (size_t)live * 4, hipMemcpyDeviceToDevice, st));
              SS_TRY(hipMemcpyAsync(d_acc_at, d_acc_at + head, (size_t)live * 4, hipMemcpyDeviceToDevice, st));
            }
            head = 0;
            tail = live;
          }
          { const int32_t rc = top_up(need); if (rc != MIDAS_SNPS_OK) return rc; }
          SS_TRY(hipEventRecord(e[5], st));
          hipLaunchKernelGGL(rs_hits_kernel, dim3(nblocks(need, 256)), dim3(256), 0, st, d_acc + head, d_cm, d_k, (uint32_t)e0,
                             (unsigned long long)N, (unsigned long long)need);
          SS_TRY(hipGetLastError());
          SS_TRY(hipEventRecord(e[6], st));
          SS_TRY(hipMemcpyAsync(&last_at, d_acc_at + head + need - 1, 4, hipMemcpyDeviceToHost, st));
          SS_TRY(hipStreamSynchronize(st));
          { const int32_t rc = lap(5, 6, 3); if (rc != MIDAS_SNPS_OK) return rc; }
          head += need;
          led.take(need);
          while (starts.size() > led.chunks.size()) starts.pop_front();
        }
        r0 = r1;
      }
    }
    SS_TRY(hipEventRecord(e[5], st));
    hipLaunchKernelGGL(rs_write_kernel, dim3(nb), dim3(256), 0, st, rp);
    SS_TRY(hipGetLastError());
    SS_TRY(hipEventRecord(e[6], st));
    hipLaunchKernelGGL(rs_pool_kernel, dim3(nb), dim3(256), 0, st, rp);
    SS_TRY(hipGetLastError());
    SS_TRY(hipEventRecord(e[7], st));
    pending = true;
    return MIDAS_SNPS_OK;
  }

  // the caller has synchronised behind run(): its last two phases are timed
  int32_t collect() {
    if (!pending) return MIDAS_SNPS_OK;
    pending = false;
    { const int32_t rc = lap(5, 6, 3); if (rc != MIDAS_SNPS_OK) return rc; }
    return lap(6, 7, 4);
  }

  // The state numpy's own loop leaves: right behind the last accepted word used -- rejected words before it are consumed, no
  // word after it is.  The chunk it came from is generated again from the state the chunk started with, up to that word, with
  // nothing written.  out_draw8: [0] raw words generated, [1] accepted words used, [2] raw words consumed, [3..7] ms.
  int32_t finish(uint32_t* key_out, int32_t* pos_out, double* out_draw8, int64_t* stats) {
    hipStream_t st = rg.st;
    std::array<uint32_t, 625> end = first;
    long long consumed = 0;
    if (led.used > 0) {
      int64_t idx = 0;
      const int k = led.last_chunk(&idx);
      if (k < 0) return ss_fail(ctx, MIDAS_SNPS_ERR_HIP, "resampling: the last draw lies in no chunk");
      const DrawChunk* c = &led.chunks[(size_t)k];
      SS_TRY(hipMemcpyAsync(d_state, starts[(size_t)k].data(), 625 * 4, hipMemcpyHostToDevice, st));
      SS_TRY(launch_mt_stream(d_state, (long long)last_at + 1, nullptr, nullptr, nullptr, 0, 0, st));
      SS_TRY(hipMemcpyAsync(end.data(), d_state, 625 * 4, hipMemcpyDeviceToHost, st));
      SS_TRY(hipStreamSynchronize(st));
      consumed = c->raw_begin + (long long)last_at + 1;
    }
    unsigned long long n_redo = 0;
    SS_TRY(hipMemcpy(&n_redo, d_n_redo, 8, hipMemcpyDeviceToHost));
    resampled = (long long)n_redo;
    for (int i = 0; i < 624; ++i) key_out[i] = end[(size_t)i];
    *pos_out = (int32_t)end[624];
    stats[11] = resampled;
    stats[12] = cells_drew;
    if (out_draw8) {
      out_draw8[0] = (double)led.raw_made; out_draw8[1] = (double)led.used; out_draw8[2] = (double)consumed;
      for (int i = 0; i < 5; ++i) out_draw8[3 + i] = ms[i];
    }
    return MIDAS_SNPS_OK;
  }
};

}  // namespace
}  // namespace midas
