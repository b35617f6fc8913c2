// gene_curves.py on MI355X (midas_genes_curves): how the pangenome grows and the core genome shrinks as samples are added, for
// the listed order of the samples and for random orders, from genes_copynum.txt as text.
//
// The contract.  Only genes_copynum.txt is read.  Rows, widths, the cell converter and the two errors are compare_genes.py's
// (genes_rows.h); an error is the earliest in file order whatever the row groups are.
//   presence   gene g, sample s: value > cutoff
//   orders     int32 [R][N], the caller's: row 0 lists the N used columns, every other row is a permutation of them; the entry
//              point checks that on the host before any device work, so the kernels index the planes with checked columns
//   need       int32 [N + 1], the caller's: 1 <= need[k] <= k, the fewest of the first k samples a core gene is present in
//   counts     c(g, r, k) = the number of the first k samples of order r in which g is present, k = 1 .. N
//              pan[r][k-1] = #{g: c >= 1}, core[r][k-1] = #{g: c >= need[k]}, single[r][k-1] = #{g: c == 1}: int64 [R][N]
// Every row read counts.  Every output is an integer and no bit of it depends on group_rows, chunk_bytes, form or a tile.
//
// The steps.
//   parse      per row group, GeneRows (genes_rows.h); the cells sample-major [sample][row]
//   planes     form 1: planes_by_sample_kernel<1, PresentCell> (bit_planes.h): [sample][W] words of 64 genes, pad bits 0
//   curves     form 1, gv_curve_kernel<B>: a workgroup owns one order and 256 consecutive gene words, a wave 64 of them, a lane
//              one.  A lane keeps its 64 genes' counts as B bit planes in registers (a vertical counter, B = 7, 10 or 13 planes
//              for N up to 127, 1 023, 8 191).  Step k loads the wave's 512 contiguous bytes of the plane of sample
//              order[r][k] (the next step's word is fetched before this step's arithmetic), adds the word by a ripple carry and
//              forms pan = OR of the planes, single = plane 0 and no other, core = the bit-sliced compare with need[k] from the
//              low bit up.  The three popcounts are summed over the wave and added by lane 0 to the workgroup's LDS accumulators
//              of the step (kSeg steps at a time), which the workgroup adds to the [R][N] accumulators with integer atomics
//              when the segment ends: exact and order-free.
//              form 0, gv_walk_kernel: a thread a (order, gene) walks the order with a plain integer count over the parsed
//              cells; the three conditions are balloted and lane 0 adds the counts to the same accumulators.
// The counts add over genes, so each row group is handled on its own and only the orders, need[] and the accumulators stay.
// No fp arithmetic beyond the cell parse, which pandas_f64.h spells with __dmul_rn / __ddiv_rn; the rest compares.
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

constexpr int kGvMaxUsed = 8191;            // the widest counter has 13 planes
constexpr long long kGvMaxOrders = 100001;  // the listed order and 100 000 random ones
constexpr int kGvSeg = 2048;                // steps whose sums a workgroup keeps in LDS at a time
constexpr int kGvWords = 256;               // gene words a workgroup: one a lane

struct GvP {
  const int32_t* orders;       // [R][N]
  const int32_t* need;         // [N + 1]
  long long R;
  int N;
  unsigned long long *pan, *core, *single;      // [R][N]
};

__device__ __forceinline__ uint32_t gv_wave_sum(uint32_t v) {
  for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
  return v;
}

// form 1: blockIdx.x = the order, blockIdx.y = 256 gene words of the group's n_words; plane [sample][wstride]
template <int B>
__global__ __launch_bounds__(256) void gv_curve_kernel(GvP p, const unsigned long long* plane, long long wstride, long long n_words) {
  __shared__ uint32_t acc[3][kGvSeg];
  const int lane = threadIdx.x & 63;
  const long long r = blockIdx.x, w = (long long)blockIdx.y * kGvWords + threadIdx.x;
  const bool mine = w < n_words;
  const int32_t* ord = p.orders + r * p.N;
  unsigned long long c[B];
#pragma unroll
  for (int b = 0; b < B; ++b) c[b] = 0ull;
  unsigned long long next = mine ? plane[(long long)ord[0] * wstride + w] : 0ull;
  for (int k0 = 0; k0 < p.N; k0 += kGvSeg) {
    const int k1 = min(p.N, k0 + kGvSeg);
    for (int i = threadIdx.x; i < k1 - k0; i += 256) { acc[0][i] = 0u; acc[1][i] = 0u; acc[2][i] = 0u; }
    __syncthreads();
    for (int k = k0; k < k1; ++k) {
      unsigned long long carry = next;
      if (k + 1 < p.N) next = mine ? plane[(long long)ord[k + 1] * wstride + w] : 0ull;
      const unsigned need = (unsigned)p.need[k + 1];
      unsigned long long any = 0ull, upper = 0ull, ge = ~0ull;
#pragma unroll
      for (int b = 0; b < B; ++b) {
        const unsigned long long t = c[b] & carry;
        c[b] ^= carry;
        carry = t;
        any |= c[b];
        if (b > 0) upper |= c[b];
        ge = ((need >> b) & 1u) ? (c[b] & ge) : (c[b] | ge);
      }
      const uint32_t n_pan = (uint32_t)__popcll(any), n_core = (uint32_t)__popcll(ge), n_single = (uint32_t)__popcll(c[0] & ~upper);
      const uint32_t two = gv_wave_sum(n_pan | (n_core << 16)), one = gv_wave_sum(n_single);      // each sum is at most 4 096
      if (lane == 0) {
        atomicAdd(&acc[0][k - k0], two & 0xFFFFu);
        atomicAdd(&acc[1][k - k0], two >> 16);
        atomicAdd(&acc[2][k - k0], one);
      }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < k1 - k0; i += 256) {
      const long long at = r * p.N + k0 + i;
      if (acc[0][i]) atomicAdd(p.pan + at, (unsigned long long)acc[0][i]);
      if (acc[1][i]) atomicAdd(p.core + at, (unsigned long long)acc[1][i]);
      if (acc[2][i]) atomicAdd(p.single + at, (unsigned long long)acc[2][i]);
    }
    __syncthreads();
  }
}

// form 0: a thread a (order, row) of the group's g rows, 256 rows of one order a workgroup pass; val [sample][stride]
__global__ __launch_bounds__(256) void gv_walk_kernel(GvP p, const double* val, long long stride, long long g, double cutoff) {
  const long long per_order = (g + 255) / 256, total = p.R * per_order;
  const int lane = threadIdx.x & 63;
  for (long long item = blockIdx.x; item < total; item += gridDim.x) {
    const long long r = item / per_order, row = (item % per_order) * 256 + threadIdx.x;
    const int32_t* ord = p.orders + r * p.N;
    int c = 0;
    for (int k = 0; k < p.N; ++k) {
      if (row < g && val[(long long)ord[k] * stride + row] > cutoff) ++c;
      const int n_pan = __popcll(__ballot(c >= 1)), n_core = __popcll(__ballot(c >= p.need[k + 1])), n_single = __popcll(__ballot(c == 1));
      if (lane == 0) {
        const long long at = r * p.N + k;
        if (n_pan) atomicAdd(p.pan + at, (unsigned long long)n_pan);
        if (n_core) atomicAdd(p.core + at, (unsigned long long)n_core);
        if (n_single) atomicAdd(p.single + at, (unsigned long long)n_single);
      }
    }
  }
}

// the rules of orders[] and need[] -> "" or the message of the first one broken
std::string gv_check(const int32_t* orders, long long R, int N, int S, const int32_t* need) {
  char buf[200];
  std::vector<long long> seen((size_t)S, -1);      // the last row in which the column stood
  std::vector<uint8_t> member((size_t)S, 0);
  for (long long r = 0; r < R; ++r)
    for (int k = 0; k < N; ++k) {
      const int32_t s = orders[r * N + k];
      const char* what = nullptr;
      if (s < 0 || s >= S) what = "is no sample column in use";
      else if (r > 0 && !member[(size_t)s]) what = "is not in row 0";
      else if (seen[(size_t)s] == r) what = "stands twice";
      if (what) {
        snprintf(buf, sizeof buf, "orders, row %lld, entry %d: the column %d %s", r, k, (int)s, what);
        return buf;
      }
      seen[(size_t)s] = r;
      if (r == 0) member[(size_t)s] = 1;
    }
  for (int k = 1; k <= N; ++k)
    if (need[k] < 1 || need[k] > k) {
      snprintf(buf, sizeof buf, "need, row %d: %d is not in [1, %d]", k, (int)need[k], k);
      return buf;
    }
  return "";
}

}  // namespace
}  // namespace midas

using namespace midas;

extern "C" {

int32_t midas_genes_curves(midas_snps_ctx* ctx, const char* text, int64_t text_bytes, int64_t n_rows_max, int32_t n_samples,
                           int32_t n_columns, const int32_t* orders, int64_t n_orders, int32_t n_used, const int32_t* need, double cutoff,
                           const int64_t* iparams8, int64_t* out_pan, int64_t* out_core, int64_t* out_single, int64_t* out_stats16,
                           float* out_ms8) {
  if (n_rows_max > 0x7FFFFFFFll || !iparams8 || !orders || !need || n_orders < 1 || n_orders > kGvMaxOrders || n_used < 1 ||
      n_used > kGvMaxUsed || n_used > n_samples || iparams8[2] < 0 || iparams8[2] > 1 || !out_pan || !out_core || !out_single)
    return MIDAS_SNPS_ERR_INVALID_ARG;
  {
    const int32_t rc = genes_begin(ctx, text, text_bytes, n_rows_max, n_samples, n_columns, iparams8, out_stats16, out_ms8);
    if (rc != MIDAS_SNPS_OK) return rc;
  }
  const int S = n_samples, N = n_used, form = (int)iparams8[2], B = N <= 127 ? 7 : N <= 1023 ? 10 : 13;
  const long long R = n_orders;
  {
    const std::string broken = gv_check(orders, R, N, S, need);
    if (!broken.empty()) return ss_fail(ctx, MIDAS_SNPS_ERR_INVALID_ARG, broken.c_str());
  }
  const size_t n_acc = (size_t)R * (size_t)N;
  out_stats16[11] = N;
  out_stats16[12] = R;
  out_stats16[13] = form;
  out_stats16[14] = form ? B : 0;
  if (n_rows_max == 0 || text_bytes == 0) {
    for (size_t k = 0; k < n_acc; ++k) { out_pan[k] = 0; out_core[k] = 0; out_single[k] = 0; }
    return MIDAS_SNPS_OK;
  }
  SS_TRY(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  SsBufs dev;
  SsEvents ev;
  float ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};     // upload + index (host clock), index, parse, planes, curves, -, -, download
  // ---- what stays: the orders, need[], the accumulators -------------------------------------------------------------------------
  {
    size_t free_b = 0, total_b = 0;
    SS_TRY(hipMemGetInfo(&free_b, &total_b));
    const size_t need_b = n_acc * (4 + 3 * 8);
    if (need_b > free_b / 4) {
      char buf[200];
      snprintf(buf, sizeof buf, "%lld orders of %d samples take %zu bytes on the device, more than a quarter of its free memory: lower --permutations",
               R, N, need_b);
      return ss_fail(ctx, MIDAS_SNPS_ERR_OUT_OF_MEMORY, buf);
    }
  }
  GvP p;
  int32_t *d_orders = nullptr, *d_need = nullptr;
  SS_TRY(dev.get(&d_orders, n_acc * 4));
  SS_TRY(dev.get(&d_need, ((size_t)N + 1) * 4));
  SS_TRY(dev.get(&p.pan, n_acc * 8));
  SS_TRY(dev.get(&p.core, n_acc * 8));
  SS_TRY(dev.get(&p.single, n_acc * 8));
  SS_TRY(hipMemcpyAsync(d_orders, orders, n_acc * 4, hipMemcpyHostToDevice, st));
  SS_TRY(hipMemcpyAsync(d_need, need, ((size_t)N + 1) * 4, hipMemcpyHostToDevice, st));
  SS_TRY(hipMemsetAsync(p.pan, 0, n_acc * 8, st));
  SS_TRY(hipMemsetAsync(p.core, 0, n_acc * 8, st));
  SS_TRY(hipMemsetAsync(p.single, 0, n_acc * 8, st));
  p.orders = d_orders; p.need = d_need; p.R = R; p.N = N;
  // ---- the walk ------------------------------------------------------------------------------------------------------------------
  GeneRows rows(ctx, dev, ev, ms, out_stats16);
  {
    const int32_t rc = rows.init(text, text_bytes, n_rows_max, S, n_columns, iparams8[0], iparams8[1], (long long)S * 8 + (S + 7) / 8 + 4, 0);
    if (rc != MIDAS_SNPS_OK) return rc;
  }
  const long long G = rows.G, wstride = (G + 63) / 64;
  if ((wstride + kGvWords - 1) / kGvWords > 65535) return ss_fail(ctx, MIDAS_SNPS_ERR_UNSUPPORTED, "a row group beyond 2^30 rows: lower group_rows");
  unsigned long long* d_bits = nullptr;
  if (form) SS_TRY(dev.get(&d_bits, (size_t)S * (size_t)wstride * 8));
  for (;;) {
    long long g = 0;
    {
      const int32_t rc = rows.next(&g);
      if (rc != MIDAS_SNPS_OK) return rc;
    }
    if (g == 0) break;
    // (queued behind the parse: a group with a bad row adds to sums nobody downloads)
    const long long n_words = (g + 63) / 64;
    if (form) {
      hipLaunchKernelGGL((planes_by_sample_kernel<1, PresentCell>), dim3((unsigned)n_words, (unsigned)((S + 3) / 4)), dim3(256), 0, st,
                         PresentCell{rows.d_val, G, cutoff}, g, S, wstride, d_bits, (unsigned long long*)nullptr);
      SS_TRY(hipGetLastError());
      SS_TRY(hipEventRecord(ev.e[4], st));
      const dim3 grid((unsigned)R, nblocks(n_words, kGvWords));
      if (B == 7) hipLaunchKernelGGL(gv_curve_kernel<7>, grid, dim3(256), 0, st, p, d_bits, wstride, n_words);
      else if (B == 10) hipLaunchKernelGGL(gv_curve_kernel<10>, grid, dim3(256), 0, st, p, d_bits, wstride, n_words);
      else hipLaunchKernelGGL(gv_curve_kernel<13>, grid, dim3(256), 0, st, p, d_bits, wstride, n_words);
    } else {
      SS_TRY(hipEventRecord(ev.e[4], st));
      const long long want = R * ((g + 255) / 256);
      hipLaunchKernelGGL(gv_walk_kernel, dim3((unsigned)std::min<long long>(want, 1 << 20)), dim3(256), 0, st, p, rows.d_val, G, g, cutoff);
    }
    SS_TRY(hipGetLastError());
    SS_TRY(hipEventRecord(ev.e[5], st));
    {
      const int32_t rc = rows.check(g);
      if (rc != MIDAS_SNPS_OK) return rc;
    }
    SS_TRY(rows.lap(3, 4, 3));
    SS_TRY(rows.lap(4, 5, 4));
    out_stats16[8] = n_words;
    rows.advance(g);
  }
  // ---- download ------------------------------------------------------------------------------------------------------------------
  SS_TRY(hipEventRecord(ev.e[0], st));
  SS_TRY(hipMemcpyAsync(out_pan, p.pan, n_acc * 8, hipMemcpyDeviceToHost, st));
  SS_TRY(hipMemcpyAsync(out_core, p.core, n_acc * 8, hipMemcpyDeviceToHost, st));
  SS_TRY(hipMemcpyAsync(out_single, p.single, n_acc * 8, hipMemcpyDeviceToHost, st));
  SS_TRY(hipEventRecord(ev.e[1], st));
  SS_TRY(hipStreamSynchronize(st));
  SS_TRY(rows.lap(0, 1, 7));
  rows.end(out_ms8);
  return MIDAS_SNPS_OK;
}

// table 0, the curves: samples, pan, core, single of order 0, new = pan[k] - pan[k - 1] and, with n_perms > 0, pan_mean pan_min
//   pan_max core_mean core_min core_max single_mean single_min single_max new_mean from means [4][n_used] (pan, core, single, new)
//   and minmax [6][n_used] (pan min, max, core min, max, single min, max), one row a k = 1 .. n_used.
// table 1, the orders: order, samples, sample_id, pan, core, single, one row an (order, k).
// The doubles are the caller's and are written as str() writes them.
int32_t midas_genes_curves_write(const char* path, const midas_genes_matrix* m, int32_t table, int64_t n_orders, int32_t n_used,
                                 const int64_t* pan, const int64_t* core, const int64_t* single, const int32_t* orders, int64_t n_perms,
                                 const double* means, const int64_t* minmax, char* err1024) {
  if (!path || !m || table < 0 || table > 1 || n_orders < 1 || n_used < 1 || !pan || !core || !single || n_perms < 0 ||
      (table == 1 && !orders) || (table == 0 && n_perms > 0 && (!means || !minmax)))
    return MIDAS_SNPS_ERR_INVALID_ARG;
  const int64_t N = n_used, n_ids = (int64_t)m->id_off.size() - 1;
  if (table == 1)
    for (int64_t k = 0; k < n_orders * N; ++k)
      if (orders[k] < 0 || orders[k] >= n_ids) return MIDAS_SNPS_ERR_INVALID_ARG;
  if (err1024) err1024[0] = 0;
  TableWriter w(path);
  if (!w.f) { gm_fail(err1024, path, 0, "cannot be written"); return MIDAS_SNPS_ERR_INVALID_ARG; }
  std::string& buf = w.buf;
  if (table == 0) {
    buf += "samples\tpan\tcore\tsingle\tnew";
    if (n_perms > 0) buf += "\tpan_mean\tpan_min\tpan_max\tcore_mean\tcore_min\tcore_max\tsingle_mean\tsingle_min\tsingle_max\tnew_mean";
    buf.push_back('\n');
    for (int64_t k = 0; k < N; ++k) {
      const int64_t v[5] = {k + 1, pan[k], core[k], single[k], pan[k] - (k > 0 ? pan[k - 1] : 0)};
      for (int c = 0; c < 5; ++c) { if (c) buf.push_back('\t'); w.i64(v[c]); }
      if (n_perms > 0) {
        for (int c = 0; c < 3; ++c) {
          buf.push_back('\t');
          w.f64(means[c * N + k]);
          buf.push_back('\t');
          w.i64(minmax[(2 * c) * N + k]);
          buf.push_back('\t');
          w.i64(minmax[(2 * c + 1) * N + k]);
        }
        buf.push_back('\t');
        w.f64(means[3 * N + k]);
      }
      w.row_done();
    }
  } else {
    buf += "order\tsamples\tsample_id\tpan\tcore\tsingle\n";
    for (int64_t r = 0; r < n_orders; ++r)
      for (int64_t k = 0; k < N; ++k) {
        const int64_t at = r * N + k, s = orders[at];
        w.i64(r);
        buf.push_back('\t');
        w.i64(k + 1);
        buf.push_back('\t');
        buf.append(m->id_pool.data() + m->id_off[(size_t)s], (size_t)(m->id_off[(size_t)s + 1] - m->id_off[(size_t)s]));
        const int64_t v[3] = {pan[at], core[at], single[at]};
        for (int c = 0; c < 3; ++c) { buf.push_back('\t'); w.i64(v[c]); }
        w.row_done();
      }
  }
  if (!w.close()) { gm_fail(err1024, path, 0, "cannot be written"); return MIDAS_SNPS_ERR_INVALID_ARG; }
  return MIDAS_SNPS_OK;
}

}  // extern "C"
