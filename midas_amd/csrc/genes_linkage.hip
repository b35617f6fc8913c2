// gene_linkage.py on MI355X (midas_genes_linkage): the pairs of genes that are present in the same samples, and the groups those
// pairs form, from genes_copynum.txt as text.
//
// The contract.  Only genes_copynum.txt is read.  Rows, widths, the cell converter and the two errors are compare_genes.py's
// (genes_rows.h); an error is the earliest in file order whatever the row groups are.
//   presence   gene g, sample s: value > cutoff.  c_g = the number of the S used samples in which g is present
//   kept       g is kept when c_g >= min_present (>= 1) and S - c_g >= min_absent; kept genes get slots 0 .. K-1 in file order
//   pairs      for kept slots a < b: both = popc(P_a & P_b) over the W = ceil(S / 64) words (the pad bits of the last word are
//              0), either = c_a + c_b - both (>= 1); the pair is linked when (double)both / (double)either >= T.  The device
//              never sees T: the host hands it need[u], u = 0 .. S, the smallest n in [0, u] with (double)n / (double)u >= T
//              (bisection over that very expression; need[0] is never used), and the kernel tests both >= need[either]
//   output     the linked pairs as three int32 arrays (slot a, slot b, both), ascending a, then ascending b; no bit and no
//              position depends on group_rows, chunk_bytes or a tile.  More than max_pairs linked pairs is
//              MIDAS_SNPS_ERR_OUT_OF_MEMORY with the exact total in out_stats16[11] and nothing written to the pair arrays
//   groups     label[k] = the smallest slot of the connected component of slot k in the graph of linked pairs (single linkage);
//              a singleton has its own slot
//
// The steps.
//   parse      per row group, GeneRows (genes_rows.h): the walk, the line index and gc_parse_kernel; the cells sample-major
//              [sample][row]
//   planes     planes_by_row_kernel over PresentCell (bit_planes.h): a workgroup takes 64 rows x 64 samples: a wave ballots a
//              sample's 64 rows, the 64 x 64 bit block is turned in LDS and written gene-major [row][W]; then c_g and the keep flag a
//              row, the library's exclusive scan of the flags, and a gather into the resident packed [K][W], count[K] and
//              row_of_slot[K], appended behind the groups before
//   pairs      a 256-thread workgroup owns a strip of 64 anchor slots, their words and counts in LDS, need[] beside them.  It
//              walks the partner slots from the strip's first to the last slot, 256 a step; a lane holds its partner's words in
//              registers (1, 2, 4, 8 or 16 of them; beyond 16 words both sides are read word by word from memory) and forms
//              `both` for each anchor in turn; the hit is balloted.  The kernel runs twice over the same code: the count pass
//              leaves the linked pairs of every anchor (only the strip's workgroup writes them: plain stores), the library's scan
//              turns them into row starts, and the write pass places a lane's pair at its anchor's cursor + the hits of the
//              waves before it + the hits below its own bit: ascending b by construction.  The count pass also leaves one bit a
//              (strip, step) that met a pair, and the write pass skips the other steps.  The strips start at blockIdx 0 with the
//              longest walk
//   labels     label = own slot; then rounds of a hook pass over the pairs (atomicMin of the smaller label on the slot the
//              larger label names), one pointer jump a slot, and a changed flag read back, until a round changes nothing.  At
//              that point every label is a root, both ends of every pair carry the same one, and a label never exceeds its
//              slot: it is the component's smallest slot, whatever order the atomics took
// No fp arithmetic beyond the cell parse, which pandas_f64.h spells with __dmul_rn / __ddiv_rn.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <string_view>
#include <vector>

#include "../../include/midas_snps.h"
#include "ctx_internal.h"
#include "genes_rows.h"
#include "kernels.h"
#include "text_rows.h"

namespace midas {
namespace {

constexpr int kStrip = 64;          // anchor slots a workgroup
constexpr int kStep = 256;          // partner slots a step: one a lane
constexpr int kRegWords = 16;       // the most words of a partner a lane keeps in registers
constexpr int kNeedLds = 4096;      // need[] lies in LDS while S + 1 <= this

// c[r] = samples in which row r is present; flag[r] = the row is kept
__global__ __launch_bounds__(256) void gl_keep_kernel(const unsigned long long* planes, long long g, int W, int S, int min_present,
                                                      int min_absent, int32_t* c, uint32_t* flag) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r >= g) return;
  int n = 0;
  for (int w = 0; w < W; ++w) n += __popcll(planes[r * W + w]);
  c[r] = n;
  flag[r] = (n >= min_present && S - n >= min_absent) ? 1u : 0u;
}

// a thread a (row, word): the kept rows' words, counts and rows go to slot k0 + rank[row]
__global__ __launch_bounds__(256) void gl_gather_kernel(const unsigned long long* planes, const int32_t* c, const uint32_t* flag,
                                                        const uint32_t* rank, long long g, int W, long long base_row, long long k0,
                                                        long long room, unsigned long long* packed, int32_t* count, int32_t* row_of_slot) {
  const long long at = (long long)blockIdx.x * 256 + threadIdx.x;
  if (at >= g * W) return;
  const long long r = at / W;
  const int w = (int)(at - r * W);
  if (!flag[r]) return;
  const long long slot = k0 + rank[r];
  if (slot >= room) return;             // (never: a slot's number is below its row's)
  packed[slot * W + w] = planes[at];
  if (w == 0) {
    count[slot] = c[r];
    row_of_slot[slot] = (int32_t)(base_row + r);
  }
}

struct GlPairP {
  const unsigned long long* planes;   // [K][W]
  const int32_t* count;               // [K]
  const int32_t* need;                // [S + 1]
  long long K, cap;                   // kept genes; entries of the pair arrays
  int W, S;
  uint32_t* row_count;                // count pass: [K] linked pairs of every anchor
  uint32_t* step_hits;                // [strips][hit_stride] bit s of a strip: its step s links a pair (count pass: set; write pass: read)
  long long hit_stride;
  unsigned long long* total;          // count pass: += them
  const uint32_t* row_start;          // write pass: [K] the exclusive scan of row_count
  int32_t *out_a, *out_b, *out_both;  // write pass
};

// kW > 0: a lane keeps kW words of its partner in registers and the strip's words lie in LDS (W <= kW); kW == 0: any W, both
// sides word by word from memory.  kWrite: the write pass.
template <int kW, bool kWrite>
__global__ __launch_bounds__(256) void gl_pairs_kernel(GlPairP q) {
  constexpr int kWs = kW > 0 ? kW : 1;
  __shared__ unsigned long long s_aw[kStrip * kWs];
  __shared__ int s_ca[kStrip];
  __shared__ int s_need[kNeedLds];
  __shared__ unsigned long long s_bal[2][4][kStrip];     // [step parity][wave][anchor]: the wave's ballot
  __shared__ uint32_t s_cursor[kStrip];
  __shared__ uint32_t s_cnt[4][kStrip];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, W = q.W;
  const long long a0 = (long long)blockIdx.x * kStrip, K = q.K;
  const int n_anchor = K - a0 < kStrip ? (int)(K - a0) : kStrip;
  const bool need_lds = q.S < kNeedLds;
  const unsigned long long* pl = q.planes;
  if (kW > 0)
    for (int e = tid; e < kStrip * kW; e += 256) {
      const int i = e / kWs, w = e % kWs;
      s_aw[e] = (i < n_anchor && w < W) ? pl[(a0 + i) * W + w] : 0ull;
    }
  if (tid < kStrip) {
    s_ca[tid] = tid < n_anchor ? q.count[a0 + tid] : 0;
    if (kWrite) s_cursor[tid] = tid < n_anchor ? q.row_start[a0 + tid] : 0u;
  }
  if (need_lds)
    for (int e = tid; e <= q.S; e += 256) s_need[e] = q.need[e];
  __syncthreads();
  uint32_t mine = 0;                  // count pass, lane i of a wave: the pairs of anchor i its wave has met
  uint32_t* const step_hits = q.step_hits + (long long)blockIdx.x * q.hit_stride;
  int step = 0, taken = 0;            // write pass: the steps it did not skip
  for (long long b0 = a0; b0 < K; b0 += kStep, ++step) {
    if (kWrite && !((step_hits[step >> 5] >> (step & 31)) & 1u)) continue;      // (the whole workgroup: the count pass met no pair here)
    const long long b = b0 + tid;
    const bool live = b < K;
    unsigned long long pw[kWs];
#pragma unroll
    for (int w = 0; w < kWs; ++w) pw[w] = (kW > 0 && live && w < W) ? pl[b * W + w] : 0ull;
    const int cb = live ? q.count[b] : 0;
    auto both_of = [&](int i) {
      int both = 0;
      if (kW > 0) {
#pragma unroll
        for (int w = 0; w < kWs; ++w) both += __popcll(s_aw[i * kWs + w] & pw[w]);
      } else if (live) {
        const unsigned long long *pa = pl + (a0 + i) * W, *pb = pl + b * W;
        for (int w = 0; w < W; ++w) both += __popcll(pa[w] & pb[w]);
      }
      return both;
    };
    unsigned long long hits = 0, my_word = 0;     // write pass: bit i: linked to anchor i; lane i: the wave's ballot of anchor i
    unsigned long long any_word = 0;              // count pass: the wave's ballots of the step, or-ed
    for (int i = 0; i < n_anchor; ++i) {
      const int both = both_of(i);
      const int either = s_ca[i] + cb - both;
      const int nd = need_lds ? s_need[either] : q.need[either];
      const bool hit = live && b > a0 + i && both >= nd;
      const unsigned long long word = __ballot(hit);
      if (kWrite) {
        if (hit) hits |= 1ull << i;
        if (lane == i) my_word = word;
      } else {
        any_word |= word;
        if (lane == i) mine += (uint32_t)__popcll(word);
      }
    }
    if (!kWrite && any_word != 0ull && lane == 0) atomicOr(&step_hits[step >> 5], 1u << (step & 31));
    if (kWrite) {
      const int par = taken++ & 1;
      s_bal[par][wave][lane] = my_word;
      if (__syncthreads_or(hits != 0ull)) {
        while (hits) {
          const int i = __ffsll((long long)hits) - 1;
          hits &= hits - 1;
          uint32_t at = s_cursor[i];
          for (int v = 0; v < wave; ++v) at += (uint32_t)__popcll(s_bal[par][v][i]);
          at += (uint32_t)__popcll(s_bal[par][wave][i] & ((1ull << lane) - 1ull));
          if ((long long)at < q.cap) {
            q.out_a[at] = (int32_t)(a0 + i);
            q.out_b[at] = (int32_t)b;
            q.out_both[at] = both_of(i);
          }
        }
        __syncthreads();
        // (the next store to s_bal[par] is two taken steps on, behind the next taken step's barrier)
        if (tid < kStrip)
          s_cursor[tid] += (uint32_t)(__popcll(s_bal[par][0][tid]) + __popcll(s_bal[par][1][tid]) + __popcll(s_bal[par][2][tid]) +
                                      __popcll(s_bal[par][3][tid]));
      }
    }
  }
  if (!kWrite) {
    s_cnt[wave][lane] = mine;
    __syncthreads();
    if (tid < n_anchor) {
      const uint32_t n = s_cnt[0][tid] + s_cnt[1][tid] + s_cnt[2][tid] + s_cnt[3][tid];
      q.row_count[a0 + tid] = n;
      if (n) atomicAdd(q.total, (unsigned long long)n);
    }
  }
}

template <bool kWrite>
void gl_launch_pairs(int form, unsigned strips, hipStream_t st, const GlPairP& q) {
  switch (form) {
    case 1: hipLaunchKernelGGL((gl_pairs_kernel<1, kWrite>), dim3(strips), dim3(256), 0, st, q); break;
    case 2: hipLaunchKernelGGL((gl_pairs_kernel<2, kWrite>), dim3(strips), dim3(256), 0, st, q); break;
    case 4: hipLaunchKernelGGL((gl_pairs_kernel<4, kWrite>), dim3(strips), dim3(256), 0, st, q); break;
    case 8: hipLaunchKernelGGL((gl_pairs_kernel<8, kWrite>), dim3(strips), dim3(256), 0, st, q); break;
    case 16: hipLaunchKernelGGL((gl_pairs_kernel<16, kWrite>), dim3(strips), dim3(256), 0, st, q); break;
    default: hipLaunchKernelGGL((gl_pairs_kernel<0, kWrite>), dim3(strips), dim3(256), 0, st, q); break;
  }
}

__global__ __launch_bounds__(256) void gl_label_init_kernel(int32_t* label, long long K) {
  const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
  if (k < K) label[k] = (int32_t)k;
}

__global__ __launch_bounds__(256) void gl_hook_kernel(const int32_t* a, const int32_t* b, long long n, int32_t* label, uint32_t* changed) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  const int32_t ra = label[a[e]], rb = label[b[e]];
  if (ra == rb) return;
  atomicMin(&label[ra > rb ? ra : rb], ra > rb ? rb : ra);
  *changed = 1u;
}

__global__ __launch_bounds__(256) void gl_jump_kernel(int32_t* label, long long K, uint32_t* changed) {
  const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
  if (k >= K) return;
  const int32_t p = label[k], pp = label[p];
  if (pp == p) return;
  label[k] = pp;
  *changed = 1u;
}

// the offsets of the rows' first bytes in the matrix's body, n_rows + 1 of them
std::vector<size_t> gl_row_starts(const midas_genes_matrix* m) {
  std::vector<size_t> at;
  at.reserve((size_t)m->n_rows + 1);
  const char* s = m->base + m->body;
  const size_t n = m->size - m->body;
  for (size_t q = 0; q < n;) {
    at.push_back(q);
    const char* x = static_cast<const char*>(memchr(s + q, '\n', n - q));
    if (!x) break;
    q = (size_t)(x - s) + 1;
  }
  at.push_back(n);
  return at;
}

std::string_view gl_gene_id(const midas_genes_matrix* m, const std::vector<size_t>& at, int64_t row) {
  const char* s = m->base + m->body + at[(size_t)row];
  size_t n = at[(size_t)row + 1] - at[(size_t)row];
  const void* tab = memchr(s, '\t', n);
  if (tab) n = (size_t)(static_cast<const char*>(tab) - s);
  else {
    while (n > 0 && (s[n - 1] == '\n' || s[n - 1] == '\r')) --n;
  }
  return std::string_view(s, n);
}

}  // namespace
}  // namespace midas

using namespace midas;

extern "C" {

int32_t midas_genes_linkage(midas_snps_ctx* ctx, const char* text, int64_t text_bytes, int64_t n_rows_max, int32_t n_samples,
                            int32_t n_columns, double cutoff, const int64_t* iparams8, const int32_t* need, int64_t max_pairs,
                            int32_t* out_count, int32_t* out_row_of_slot, int32_t* out_label, int32_t* out_a, int32_t* out_b,
                            int32_t* out_both, int64_t* out_stats16, float* out_ms8) {
  if (n_rows_max > 0x7FFFFFFFll || n_samples > 65535 * 64 || !iparams8 || !need || iparams8[2] < 1 || iparams8[3] < 0 || iparams8[4] < 0 ||
      iparams8[4] > 1 || max_pairs < 0 || max_pairs > 0x7FFFFFFFll || (n_rows_max > 0 && (!out_count || !out_row_of_slot || !out_label)) ||
      (max_pairs > 0 && (!out_a || !out_b || !out_both)))
    return MIDAS_SNPS_ERR_INVALID_ARG;
  {
    const int32_t rc = genes_begin(ctx, text, text_bytes, n_rows_max, n_samples, n_columns, iparams8, out_stats16, out_ms8);
    if (rc != MIDAS_SNPS_OK) return rc;
  }
  const int S = n_samples, W = (S + 63) / 64;
  const int min_present = (int)std::min<int64_t>(iparams8[2], (int64_t)S + 1), min_absent = (int)std::min<int64_t>(iparams8[3], (int64_t)S + 1);
  if (n_rows_max == 0 || text_bytes == 0) return MIDAS_SNPS_OK;
  SS_TRY(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  SsBufs dev;
  SsEvents ev;
  float ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};     // upload + index (host clock), index, parse, planes, count pass, write pass, labels, download
  // ---- the resident side: the packed planes, counts and rows of the kept genes (at most every row), need[] ----------------------
  const size_t rows_cap = (size_t)n_rows_max;
  unsigned long long *d_packed = nullptr, *d_total = nullptr;
  int32_t *d_count = nullptr, *d_row_of_slot = nullptr, *d_need = nullptr, *d_label = nullptr;
  uint32_t *d_row_count = nullptr, *d_changed = nullptr;
  SS_TRY(dev.get(&d_packed, rows_cap * (size_t)W * 8));
  SS_TRY(dev.get(&d_count, rows_cap * 4));
  SS_TRY(dev.get(&d_row_of_slot, rows_cap * 4));
  SS_TRY(dev.get(&d_need, ((size_t)S + 1) * 4));
  SS_TRY(dev.get(&d_total, 8));
  SS_TRY(dev.get(&d_changed, 4));
  SS_TRY(hipMemcpyAsync(d_need, need, ((size_t)S + 1) * 4, hipMemcpyHostToDevice, st));
  // ---- the walk: the group's planes, its kept rows, their slots (the free memory is read behind the resident side) -------------
  GeneRows rows(ctx, dev, ev, ms, out_stats16);
  {
    const int32_t rc = rows.init(text, text_bytes, n_rows_max, S, n_columns, iparams8[0], iparams8[1],
                                 (long long)S * 8 + (long long)W * 8 + 4 + 4 + 4 + 4, n_rows_max);
    if (rc != MIDAS_SNPS_OK) return rc;
  }
  const long long G = rows.G;
  uint32_t *d_scratch = rows.d_scratch, *d_flag = nullptr, *d_rank = nullptr;
  unsigned long long* d_planes = nullptr;
  int32_t* d_c = nullptr;
  SS_TRY(dev.get(&d_planes, (size_t)G * (size_t)W * 8));
  SS_TRY(dev.get(&d_c, (size_t)G * 4));
  SS_TRY(dev.get(&d_flag, (size_t)G * 4));
  SS_TRY(dev.get(&d_rank, (size_t)G * 4));
  long long K = 0;
  for (;;) {
    long long g = 0;
    {
      const int32_t rc = rows.next(&g);
      if (rc != MIDAS_SNPS_OK) return rc;
    }
    if (g == 0) break;
    hipLaunchKernelGGL((planes_by_row_kernel<1, PresentCell>), dim3(nblocks(g, 64), (unsigned)W), dim3(256), 0, st, PresentCell{rows.d_val, G, cutoff},
                       g, S, W, d_planes, (unsigned long long*)nullptr);
    SS_TRY(hipGetLastError());
    hipLaunchKernelGGL(gl_keep_kernel, dim3(nblocks(g, 256)), dim3(256), 0, st, d_planes, g, W, S, min_present, min_absent, d_c, d_flag);
    SS_TRY(hipGetLastError());
    SS_TRY(launch_scan_u32(d_flag, d_rank, g, d_scratch, st));
    hipLaunchKernelGGL(gl_gather_kernel, dim3(nblocks(g * W, 256)), dim3(256), 0, st, d_planes, d_c, d_flag, d_rank, g, W, rows.base, K,
                       (long long)rows_cap, d_packed, d_count, d_row_of_slot);
    SS_TRY(hipGetLastError());
    SS_TRY(hipEventRecord(ev.e[4], st));
    uint32_t last_flag = 0, last_rank = 0;
    SS_TRY(hipMemcpyAsync(&last_flag, d_flag + g - 1, 4, hipMemcpyDeviceToHost, st));
    SS_TRY(hipMemcpyAsync(&last_rank, d_rank + g - 1, 4, hipMemcpyDeviceToHost, st));
    {
      const int32_t rc = rows.check(g);
      if (rc != MIDAS_SNPS_OK) return rc;
    }
    SS_TRY(rows.lap(3, 4, 3));
    K += (long long)last_flag + last_rank;
    rows.advance(g);
  }
  rows.end(nullptr);              // (the walk's statistics now: more pairs than max_pairs is an error that reports them)
  out_stats16[1] = K;
  out_stats16[8] = K * (K - 1) / 2;
  // ---- the pairs: count pass, row starts, write pass ---------------------------------------------------------------------------
  int form = 0;
  if (iparams8[4] == 0 && W <= kRegWords) for (form = 1; form < W; form *= 2) {}
  const long long strips = (K + kStrip - 1) / kStrip;
  out_stats16[13] = form;
  out_stats16[14] = strips;
  unsigned long long total = 0;
  uint32_t *d_row_start = nullptr, *d_step_hits = nullptr;
  const long long hit_stride = ((K + kStep - 1) / kStep + 31) / 32 + 1;
  int32_t *d_a = nullptr, *d_b = nullptr, *d_both = nullptr;
  GlPairP q;
  q.planes = d_packed; q.count = d_count; q.need = d_need; q.K = K; q.cap = 0; q.W = W; q.S = S; q.row_count = nullptr; q.total = d_total;
  q.step_hits = nullptr; q.hit_stride = hit_stride;
  q.row_start = nullptr; q.out_a = q.out_b = q.out_both = nullptr;
  if (K > 1) {
    SS_TRY(dev.get(&d_row_count, (size_t)K * 4));
    SS_TRY(dev.get(&d_row_start, (size_t)K * 4));
    SS_TRY(dev.get(&d_step_hits, (size_t)strips * (size_t)hit_stride * 4));
    q.row_count = d_row_count;
    q.step_hits = d_step_hits;
    SS_TRY(hipMemsetAsync(d_total, 0, 8, st));
    SS_TRY(hipMemsetAsync(d_step_hits, 0, (size_t)strips * (size_t)hit_stride * 4, st));
    SS_TRY(hipEventRecord(ev.e[0], st));
    gl_launch_pairs<false>(form, (unsigned)strips, st, q);
    SS_TRY(hipGetLastError());
    SS_TRY(hipEventRecord(ev.e[1], st));
    SS_TRY(hipMemcpyAsync(&total, d_total, 8, hipMemcpyDeviceToHost, st));
    SS_TRY(hipStreamSynchronize(st));
    SS_TRY(rows.lap(0, 1, 4));
  }
  out_stats16[11] = (int64_t)total;
  if (total > (unsigned long long)max_pairs) {
    char buf[200];
    snprintf(buf, sizeof buf, "%llu linked pairs of genes, but max_pairs is %lld", total, (long long)max_pairs);
    rows.end(out_ms8);
    return ss_fail(ctx, MIDAS_SNPS_ERR_OUT_OF_MEMORY, buf);
  }
  SS_TRY(dev.get(&d_label, (size_t)std::max<long long>(K, 1) * 4));
  if (K > 0) {
    hipLaunchKernelGGL(gl_label_init_kernel, dim3(nblocks(K, 256)), dim3(256), 0, st, d_label, K);
    SS_TRY(hipGetLastError());
  }
  long long rounds = 0;
  if (total > 0) {
    SS_TRY(dev.get(&d_a, (size_t)total * 4));
    SS_TRY(dev.get(&d_b, (size_t)total * 4));
    SS_TRY(dev.get(&d_both, (size_t)total * 4));
    q.cap = (long long)total; q.row_start = d_row_start; q.out_a = d_a; q.out_b = d_b; q.out_both = d_both;
    SS_TRY(hipEventRecord(ev.e[0], st));
    SS_TRY(launch_scan_u32(d_row_count, d_row_start, K, d_scratch, st));
    gl_launch_pairs<true>(form, (unsigned)strips, st, q);
    SS_TRY(hipGetLastError());
    SS_TRY(hipEventRecord(ev.e[1], st));
    // ---- labels: rounds of hook and jump until one changes nothing ------------------------------------------------------------
    SS_TRY(hipEventRecord(ev.e[2], st));
    for (;;) {
      uint32_t changed = 0;
      SS_TRY(hipMemsetAsync(d_changed, 0, 4, st));
      hipLaunchKernelGGL(gl_hook_kernel, dim3(nblocks((long long)total, 256)), dim3(256), 0, st, d_a, d_b, (long long)total, d_label, d_changed);
      SS_TRY(hipGetLastError());
      hipLaunchKernelGGL(gl_jump_kernel, dim3(nblocks(K, 256)), dim3(256), 0, st, d_label, K, d_changed);
      SS_TRY(hipGetLastError());
      SS_TRY(hipMemcpyAsync(&changed, d_changed, 4, hipMemcpyDeviceToHost, st));
      SS_TRY(hipStreamSynchronize(st));
      if (!changed) break;
      if (++rounds > K + 1) return ss_fail(ctx, MIDAS_SNPS_ERR_HIP, "the labels did not settle");      // (never: a label only falls)
    }
    SS_TRY(hipEventRecord(ev.e[3], st));
    SS_TRY(hipStreamSynchronize(st));
    SS_TRY(rows.lap(0, 1, 5));
    SS_TRY(rows.lap(2, 3, 6));
  }
  out_stats16[12] = rounds;
  // ---- download ----------------------------------------------------------------------------------------------------------------
  SS_TRY(hipEventRecord(ev.e[0], st));
  if (K > 0) {
    SS_TRY(hipMemcpyAsync(out_count, d_count, (size_t)K * 4, hipMemcpyDeviceToHost, st));
    SS_TRY(hipMemcpyAsync(out_row_of_slot, d_row_of_slot, (size_t)K * 4, hipMemcpyDeviceToHost, st));
    SS_TRY(hipMemcpyAsync(out_label, d_label, (size_t)K * 4, hipMemcpyDeviceToHost, st));
  }
  if (total > 0) {
    SS_TRY(hipMemcpyAsync(out_a, d_a, (size_t)total * 4, hipMemcpyDeviceToHost, st));
    SS_TRY(hipMemcpyAsync(out_b, d_b, (size_t)total * 4, hipMemcpyDeviceToHost, st));
    SS_TRY(hipMemcpyAsync(out_both, d_both, (size_t)total * 4, hipMemcpyDeviceToHost, st));
  }
  SS_TRY(hipEventRecord(ev.e[1], st));
  SS_TRY(hipStreamSynchronize(st));
  SS_TRY(rows.lap(0, 1, 7));
  rows.end(out_ms8);
  return MIDAS_SNPS_OK;
}

// gene1, gene2, count1, count2, count_both, count_either, jaccard for the linked pairs in their order
int32_t midas_genes_linkage_write_pairs(const char* path, const midas_genes_matrix* m, int64_t n_slots, const int32_t* count,
                                        const int32_t* row_of_slot, int64_t n_pairs, const int32_t* pair_a, const int32_t* pair_b,
                                        const int32_t* pair_both, char* err1024) {
  if (!path || !m || n_slots < 0 || n_pairs < 0 || (n_slots > 0 && (!count || !row_of_slot)) || (n_pairs > 0 && (!pair_a || !pair_b || !pair_both)))
    return MIDAS_SNPS_ERR_INVALID_ARG;
  if (err1024) err1024[0] = 0;
  for (int64_t k = 0; k < n_slots; ++k)
    if (row_of_slot[k] < 0 || row_of_slot[k] >= m->n_rows) return MIDAS_SNPS_ERR_INVALID_ARG;
  for (int64_t e = 0; e < n_pairs; ++e)
    if (pair_a[e] < 0 || pair_a[e] >= n_slots || pair_b[e] < 0 || pair_b[e] >= n_slots) return MIDAS_SNPS_ERR_INVALID_ARG;
  const std::vector<size_t> at = gl_row_starts(m);
  TableWriter w(path);
  if (!w.f) { gm_fail(err1024, path, 0, "cannot be written"); return MIDAS_SNPS_ERR_INVALID_ARG; }
  w.buf += "gene1\tgene2\tcount1\tcount2\tcount_both\tcount_either\tjaccard\n";
  for (int64_t e = 0; e < n_pairs; ++e) {
    const int32_t a = pair_a[e], b = pair_b[e];
    const int64_t c1 = count[a], c2 = count[b], both = pair_both[e], either = c1 + c2 - both;
    w.buf.append(gl_gene_id(m, at, row_of_slot[a]));
    w.buf.push_back('\t');
    w.buf.append(gl_gene_id(m, at, row_of_slot[b]));
    const int64_t v[4] = {c1, c2, both, either};
    for (int c = 0; c < 4; ++c) { w.buf.push_back('\t'); w.i64(v[c]); }
    w.buf.push_back('\t');
    w.f64(either != 0 ? (double)both / (double)either : 0.0);
    w.row_done();
  }
  if (!w.close()) { gm_fail(err1024, path, 0, "cannot be written"); return MIDAS_SNPS_ERR_INVALID_ARG; }
  return MIDAS_SNPS_OK;
}

// group_id, group_size, gene_id, count: the kept genes of the components of at least min_group genes; the ids count from 1 in the
// order of each component's first gene (its label), the rows go by group, then by slot
int32_t midas_genes_linkage_write_groups(const char* path, const midas_genes_matrix* m, int64_t n_slots, const int32_t* count,
                                         const int32_t* row_of_slot, const int32_t* label, int64_t min_group, int64_t* out_n_groups,
                                         char* err1024) {
  if (!path || !m || n_slots < 0 || min_group < 1 || (n_slots > 0 && (!count || !row_of_slot || !label))) return MIDAS_SNPS_ERR_INVALID_ARG;
  if (err1024) err1024[0] = 0;
  if (out_n_groups) *out_n_groups = 0;
  for (int64_t k = 0; k < n_slots; ++k)
    if (row_of_slot[k] < 0 || row_of_slot[k] >= m->n_rows || label[k] < 0 || label[k] > k) return MIDAS_SNPS_ERR_INVALID_ARG;
  // the members of a component in slot order, chained behind its label
  std::vector<int64_t> size((size_t)n_slots, 0), start((size_t)n_slots + 1, 0), fill;
  for (int64_t k = 0; k < n_slots; ++k) ++size[(size_t)label[k]];
  for (int64_t k = 0; k < n_slots; ++k) start[(size_t)k + 1] = start[(size_t)k] + size[(size_t)k];
  fill.assign(start.begin(), start.end() - 1);
  std::vector<int32_t> member((size_t)n_slots);
  for (int64_t k = 0; k < n_slots; ++k) member[(size_t)fill[(size_t)label[k]]++] = (int32_t)k;
  const std::vector<size_t> at = gl_row_starts(m);
  TableWriter w(path);
  if (!w.f) { gm_fail(err1024, path, 0, "cannot be written"); return MIDAS_SNPS_ERR_INVALID_ARG; }
  w.buf += "group_id\tgroup_size\tgene_id\tcount\n";
  int64_t id = 0;
  for (int64_t r = 0; r < n_slots; ++r) {
    if (label[r] != r || size[(size_t)r] < min_group) continue;
    ++id;
    for (int64_t x = start[(size_t)r]; x < start[(size_t)r + 1]; ++x) {
      const int32_t k = member[(size_t)x];
      w.i64(id);
      w.buf.push_back('\t');
      w.i64(size[(size_t)r]);
      w.buf.push_back('\t');
      w.buf.append(gl_gene_id(m, at, row_of_slot[k]));
      w.buf.push_back('\t');
      w.i64(count[k]);
      w.row_done();
    }
  }
  if (out_n_groups) *out_n_groups = id;
  if (!w.close()) { gm_fail(err1024, path, 0, "cannot be written"); return MIDAS_SNPS_ERR_INVALID_ARG; }
  return MIDAS_SNPS_OK;
}

}  // extern "C"
