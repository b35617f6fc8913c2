// gene_assoc.py on MI355X (midas_genes_assoc): which genes differ between two groups of samples, from genes_copynum.txt as text
// (DESIGN.md section 22).
//
// The contract.  Only genes_copynum.txt is read.  Rows, widths, the cell converter and the two errors are compare_genes.py's
// (genes_rows.h); an error is the earliest in file order whatever the row groups are.
//   samples    bit s of use[]: column s takes part; bit s of case[] (within use[]): it is a case.  N used, n1 cases, N <= 8 191
//   presence   value > cutoff; c = the used samples in which the gene is present, a = the cases among them
//   kept       c >= min_present and N - c >= min_absent; kept genes get slots 0 .. K-1 in file order
//   presabs    w = a; ties = 0; x(L) = N a(L) - n1 c
//   copynum    r_s = 2 #{t: v_t < v_s} + #{t: v_t == v_s} + 1 over the used samples (the parsed doubles compared by < and ==);
//              w = sum of r_s over the cases; ties = sum of (e_s^2 - 1), e_s = #{t: v_t == v_s}; x(L) = w(L) - n1 (N + 1)
//   exceed     the relabellings b < P (planes [P][W], bit s: sample s is a case under b) with |x(M_b)| >= |x(L0)|
//   products   where asked for, a(M_b) or w(M_b) of every kept slot and relabelling
// Every output is an integer and no bit of it depends on group_rows, chunk_bytes, form or a tile.
//
// The steps.
//   expand     once: the planes to the byte image the MFMA reads (assoc_kernels.h), at most a quarter of the free memory
//   parse      per row group, GeneRows (genes_rows.h); the cells sample-major [sample][row]
//   keep       a thread a row: c, a and the keep flag; the library's exclusive scan of the flags gives the kept rows their places
//   ranks      as_rank_kernel: the digits of the kept rows at their places in the group's image, w and ties, the slot's row and
//              counts
//   product    as_product_kernel (form 1: i8 MFMA, a workgroup owns 32 kept rows over all P) or as_walk_kernel (form 0: a thread
//              a (row, relabelling), plain adds) leaves exceed, and the products where asked for
// Between groups only the image of the relabellings and the results (28 bytes a kept gene) stay on the device.
// No fp arithmetic beyond the cell parse, which pandas_f64.h spells with __dmul_rn / __ddiv_rn; the rest compares.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <string_view>
#include <vector>

#include "../../include/midas_snps.h"
#include "assoc_kernels.h"
#include "ctx_internal.h"
#include "genes_rows.h"
#include "kernels.h"
#include "text_rows.h"

namespace midas {
namespace {

constexpr long long kAsMaxPerms = 1000000;
constexpr long long kAsMaxProducts = 1ll << 24;

// a thread a row: c = used samples in which it is present, a = cases among them, flag = the row is kept
__global__ __launch_bounds__(256) void ga_keep_kernel(const double* val, long long stride, long long g, const int32_t* col_of,
                                                      const uint8_t* is_case, int N, double cutoff, int min_present, int min_absent,
                                                      int32_t* c, int32_t* a, uint32_t* flag) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r >= g) return;
  int n = 0, m = 0;
  for (int j = 0; j < N; ++j) {
    const bool present = val[(long long)col_of[j] * stride + r] > cutoff;
    n += present ? 1 : 0;
    m += present && is_case[j] ? 1 : 0;
  }
  c[r] = n;
  a[r] = m;
  flag[r] = (n >= min_present && N - n >= min_absent) ? 1u : 0u;
}

}  // namespace
}  // namespace midas

using namespace midas;

extern "C" {

int32_t midas_genes_assoc(midas_snps_ctx* ctx, const char* text, int64_t text_bytes, int64_t n_rows_max, int32_t n_samples,
                          int32_t n_columns, const uint64_t* use_words, const uint64_t* case_words, const uint64_t* perm_planes,
                          int64_t n_perms, double cutoff, const int64_t* iparams8, int32_t* out_row_of_slot, int32_t* out_count,
                          int32_t* out_count_case, int64_t* out_w, int64_t* out_ties, uint32_t* out_exceed, int32_t* out_products,
                          int64_t* out_stats16, float* out_ms8) {
  if (n_rows_max > 0x7FFFFFFFll || n_samples > 65535 * 64 || !iparams8 || !use_words || !case_words || iparams8[2] < 0 || iparams8[3] < 0 ||
      iparams8[4] < 0 || iparams8[4] > 1 || iparams8[5] < 0 || iparams8[5] > 1 || n_perms < 0 || n_perms > kAsMaxPerms ||
      (n_perms > 0 && !perm_planes) ||
      (n_rows_max > 0 && (!out_row_of_slot || !out_count || !out_count_case || !out_w || !out_ties || !out_exceed)))
    return MIDAS_SNPS_ERR_INVALID_ARG;
  {
    const int32_t rc = genes_begin(ctx, text, text_bytes, n_rows_max, n_samples, n_columns, iparams8, out_stats16, out_ms8);
    if (rc != MIDAS_SNPS_OK) return rc;
  }
  const int S = n_samples, W = (S + 63) / 64, kind = (int)iparams8[4], form = (int)iparams8[5];
  const long long P = n_perms;
  // ---- the used samples in column order --------------------------------------------------------------------------------------
  std::vector<int32_t> col_of;
  std::vector<uint8_t> is_case;
  int n1 = 0;
  for (int s = 0; s < S; ++s) {
    if (!((use_words[s >> 6] >> (s & 63)) & 1ull)) continue;
    col_of.push_back(s);
    is_case.push_back((uint8_t)((case_words[s >> 6] >> (s & 63)) & 1ull));
    n1 += is_case.back();
  }
  if (col_of.empty()) return MIDAS_SNPS_ERR_INVALID_ARG;
  if (col_of.size() > (size_t)kAsMaxUsed) {
    char buf[160];
    snprintf(buf, sizeof buf, "%zu used samples: the doubled ranks of more than %d do not fit two 7-bit digits", col_of.size(), kAsMaxUsed);
    return ss_fail(ctx, MIDAS_SNPS_ERR_UNSUPPORTED, buf);
  }
  const int N = (int)col_of.size(), Kp = (N + 63) / 64 * 64;
  const long long Ppad = (P + 15) / 16 * 16;
  // (the products are refused when the kept rows turn out to need more than 2^24 of them: behind the group that shows it)
  const long long prod_cap = out_products ? std::min<long long>(n_rows_max * P, kAsMaxProducts) : 0;
  const int min_present = (int)std::min<int64_t>(iparams8[2], (int64_t)N + 1), min_absent = (int)std::min<int64_t>(iparams8[3], (int64_t)N + 1);
  out_stats16[11] = N;
  out_stats16[12] = n1;
  out_stats16[13] = form;
  out_stats16[14] = Kp;
  if (n_rows_max == 0 || text_bytes == 0) return MIDAS_SNPS_OK;
  SS_TRY(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  SsBufs dev;
  SsEvents ev;
  float ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};     // upload + index (host clock), index, parse, keep + ranks, product, expand, -, download
  // ---- what stays: the image of the relabellings, the results a slot -----------------------------------------------------------
  const size_t rows_cap = (size_t)n_rows_max;
  int8_t* d_img = nullptr;
  unsigned long long *d_planes = nullptr, *d_w = nullptr, *d_ties = nullptr;
  int32_t *d_col_of = nullptr, *d_row_of_slot = nullptr, *d_count = nullptr, *d_count_case = nullptr, *d_products = nullptr;
  uint8_t* d_is_case = nullptr;
  uint32_t* d_exceed = nullptr;
  if (P > 0) {
    size_t free_b = 0, total_b = 0;
    SS_TRY(hipMemGetInfo(&free_b, &total_b));
    const size_t need_b = (size_t)Ppad * (size_t)Kp + (size_t)P * (size_t)W * 8;
    if (need_b > free_b / 4) {
      char buf[200];
      snprintf(buf, sizeof buf, "%lld relabellings of %d samples take %zu bytes on the device, more than a quarter of its free memory: lower --permutations",
               P, N, need_b);
      return ss_fail(ctx, MIDAS_SNPS_ERR_OUT_OF_MEMORY, buf);
    }
    SS_TRY(dev.get(&d_img, (size_t)Ppad * (size_t)Kp));
    SS_TRY(dev.get(&d_planes, (size_t)P * (size_t)W * 8));
  }
  SS_TRY(dev.get(&d_col_of, (size_t)N * 4));
  SS_TRY(dev.get(&d_is_case, (size_t)N));
  SS_TRY(dev.get(&d_row_of_slot, rows_cap * 4));
  SS_TRY(dev.get(&d_count, rows_cap * 4));
  SS_TRY(dev.get(&d_count_case, rows_cap * 4));
  SS_TRY(dev.get(&d_w, rows_cap * 8));
  SS_TRY(dev.get(&d_ties, rows_cap * 8));
  SS_TRY(dev.get(&d_exceed, rows_cap * 4));
  if (prod_cap > 0) SS_TRY(dev.get(&d_products, (size_t)prod_cap * 4));
  SS_TRY(hipMemcpyAsync(d_col_of, col_of.data(), (size_t)N * 4, hipMemcpyHostToDevice, st));
  SS_TRY(hipMemcpyAsync(d_is_case, is_case.data(), (size_t)N, hipMemcpyHostToDevice, st));
  SS_TRY(hipMemsetAsync(d_w, 0, rows_cap * 8, st));
  SS_TRY(hipMemsetAsync(d_ties, 0, rows_cap * 8, st));
  SS_TRY(hipMemsetAsync(d_exceed, 0, rows_cap * 4, st));
  // ---- the walk ----------------------------------------------------------------------------------------------------------------
  GeneRows rows(ctx, dev, ev, ms, out_stats16);
  {
    const int32_t rc = rows.init(text, text_bytes, n_rows_max, S, n_columns, iparams8[0], iparams8[1],
                                 (long long)S * 8 + (long long)Kp * 2 + 4 + 4 + 4 + 4, n_rows_max);
    if (rc != MIDAS_SNPS_OK) return rc;
  }
  const long long G = rows.G;
  if (P > 0) {
    SS_TRY(hipMemcpyAsync(d_planes, perm_planes, (size_t)P * (size_t)W * 8, hipMemcpyHostToDevice, st));
    SS_TRY(hipEventRecord(ev.e[0], st));
    hipLaunchKernelGGL(as_expand_kernel, dim3(nblocks(Ppad * (Kp / 4), 256)), dim3(256), 0, st, d_planes, W, d_col_of, N, Kp, P, Ppad, d_img);
    SS_TRY(hipGetLastError());
    SS_TRY(hipEventRecord(ev.e[6], st));
    SS_TRY(hipStreamSynchronize(st));
    SS_TRY(rows.lap(0, 6, 5));
  }
  uint32_t *d_scratch = rows.d_scratch, *d_flag = nullptr, *d_rank = nullptr;
  int32_t *d_c = nullptr, *d_a = nullptr;
  int8_t *d_lo = nullptr, *d_hi = nullptr;
  SS_TRY(dev.get(&d_c, (size_t)G * 4));
  SS_TRY(dev.get(&d_a, (size_t)G * 4));
  SS_TRY(dev.get(&d_flag, (size_t)G * 4));
  SS_TRY(dev.get(&d_rank, (size_t)G * 4));
  SS_TRY(dev.get(&d_lo, (size_t)G * (size_t)Kp));
  if (kind) SS_TRY(dev.get(&d_hi, (size_t)G * (size_t)Kp));
  int R = 64;                                 // rows a workgroup of the rank kernel: their used values fit its LDS
  while (R > 1 && R * N > kAsMaxUsed) R /= 2;
  const size_t lds = (size_t)(kind ? 2 : 1) * kAsTile * (size_t)(Kp + 16);
  const bool in_lds = lds <= (size_t)kAsLdsBytes;
  out_stats16[8] = in_lds ? 1 : 0;
  long long K = 0;
  for (;;) {
    long long g = 0;
    {
      const int32_t rc = rows.next(&g);
      if (rc != MIDAS_SNPS_OK) return rc;
    }
    if (g == 0) break;
    hipLaunchKernelGGL(ga_keep_kernel, dim3(nblocks(g, 256)), dim3(256), 0, st, rows.d_val, G, g, d_col_of, d_is_case, N, cutoff, min_present,
                       min_absent, d_c, d_a, d_flag);
    SS_TRY(hipGetLastError());
    SS_TRY(launch_scan_u32(d_flag, d_rank, g, d_scratch, st));
    AsRankP rp;
    rp.val = rows.d_val; rp.stride = G; rp.col_of = d_col_of; rp.is_case = d_is_case; rp.N = N; rp.Kp = Kp; rp.R = R; rp.cutoff = cutoff;
    rp.flag = d_flag; rp.rank = d_rank; rp.c = d_c; rp.a = d_a; rp.g = g; rp.base_row = rows.base; rp.k0 = K; rp.room = (long long)rows_cap;
    rp.lo = d_lo; rp.hi = d_hi; rp.row_of_slot = d_row_of_slot; rp.count = d_count; rp.count_case = d_count_case; rp.w = d_w; rp.ties = d_ties;
    if (kind) hipLaunchKernelGGL(as_rank_kernel<1>, dim3(nblocks(g, R)), dim3(256), 0, st, rp);
    else hipLaunchKernelGGL(as_rank_kernel<0>, dim3(nblocks(g, R)), dim3(256), 0, st, rp);
    SS_TRY(hipGetLastError());
    SS_TRY(hipEventRecord(ev.e[4], st));
    if (P > 0) {
      AsProdP q;
      q.lo = d_lo; q.hi = d_hi; q.img = d_img; q.planes = d_planes; q.col_of = d_col_of; q.W = W; q.Kp = Kp; q.N = N; q.n1 = n1; q.P = P;
      q.last_flag = d_flag + g - 1; q.last_rank = d_rank + g - 1; q.k0 = K; q.room = (long long)rows_cap; q.count = d_count; q.w = d_w;
      q.exceed = d_exceed; q.products = d_products; q.prod_cap = prod_cap;
      const unsigned tiles = nblocks(g, kAsTile);
      if (form == 0) {
        const long long want = ((long long)g * P + 255) / 256;
        hipLaunchKernelGGL(as_walk_kernel, dim3((unsigned)std::min<long long>(want, 1 << 20)), dim3(256), 0, st, q, kind ? 0 : 1);
      } else if (kind) {
        if (in_lds) hipLaunchKernelGGL((as_product_kernel<2, true>), dim3(tiles), dim3(256), lds, st, q);
        else hipLaunchKernelGGL((as_product_kernel<2, false>), dim3(tiles), dim3(256), 0, st, q);
      } else {
        if (in_lds) hipLaunchKernelGGL((as_product_kernel<1, true>), dim3(tiles), dim3(256), lds, st, q);
        else hipLaunchKernelGGL((as_product_kernel<1, false>), dim3(tiles), dim3(256), 0, st, q);
      }
      SS_TRY(hipGetLastError());
    }
    SS_TRY(hipEventRecord(ev.e[5], st));
    uint32_t last_flag = 0, last_rank = 0;
    SS_TRY(hipMemcpyAsync(&last_flag, d_flag + g - 1, 4, hipMemcpyDeviceToHost, st));
    SS_TRY(hipMemcpyAsync(&last_rank, d_rank + g - 1, 4, hipMemcpyDeviceToHost, st));
    {
      const int32_t rc = rows.check(g);
      if (rc != MIDAS_SNPS_OK) return rc;
    }
    SS_TRY(rows.lap(3, 4, 3));
    SS_TRY(rows.lap(4, 5, 4));
    K += (long long)last_flag + last_rank;
    rows.advance(g);
    if (out_products && K * P > kAsMaxProducts) {
      rows.end(out_ms8);
      return ss_fail(ctx, MIDAS_SNPS_ERR_INVALID_ARG, "out_products: more than 2^24 products of kept genes and relabellings");
    }
  }
  rows.end(nullptr);
  out_stats16[1] = K;
  // ---- download ----------------------------------------------------------------------------------------------------------------
  SS_TRY(hipEventRecord(ev.e[0], st));
  if (K > 0) {
    SS_TRY(hipMemcpyAsync(out_row_of_slot, d_row_of_slot, (size_t)K * 4, hipMemcpyDeviceToHost, st));
    SS_TRY(hipMemcpyAsync(out_count, d_count, (size_t)K * 4, hipMemcpyDeviceToHost, st));
    SS_TRY(hipMemcpyAsync(out_count_case, d_count_case, (size_t)K * 4, hipMemcpyDeviceToHost, st));
    SS_TRY(hipMemcpyAsync(out_w, d_w, (size_t)K * 8, hipMemcpyDeviceToHost, st));
    SS_TRY(hipMemcpyAsync(out_ties, d_ties, (size_t)K * 8, hipMemcpyDeviceToHost, st));
    SS_TRY(hipMemcpyAsync(out_exceed, d_exceed, (size_t)K * 4, hipMemcpyDeviceToHost, st));
    if (out_products && P > 0) SS_TRY(hipMemcpyAsync(out_products, d_products, (size_t)(K * P) * 4, hipMemcpyDeviceToHost, st));
  }
  SS_TRY(hipEventRecord(ev.e[1], st));
  SS_TRY(hipStreamSynchronize(st));
  SS_TRY(rows.lap(0, 1, 7));
  rows.end(out_ms8);
  return MIDAS_SNPS_OK;
}

// gene_id, count_case, count_control, effect, p_value, q_value and, with n_perms > 0, exceed, p_perm, q_perm for the kept slots in
// their order; the floats are the caller's and are written as str() writes them
int32_t midas_genes_assoc_write(const char* path, const midas_genes_matrix* m, int64_t n_slots, const int32_t* row_of_slot,
                                const int32_t* count, const int32_t* count_case, const double* effect, const double* p_value,
                                const double* q_value, int64_t n_perms, const uint32_t* exceed, const double* p_perm, const double* q_perm,
                                char* err1024) {
  if (!path || !m || n_slots < 0 || n_perms < 0 || (n_slots > 0 && (!row_of_slot || !count || !count_case || !effect || !p_value || !q_value)) ||
      (n_slots > 0 && n_perms > 0 && (!exceed || !p_perm || !q_perm)))
    return MIDAS_SNPS_ERR_INVALID_ARG;
  if (err1024) err1024[0] = 0;
  for (int64_t k = 0; k < n_slots; ++k)
    if (row_of_slot[k] < 0 || row_of_slot[k] >= m->n_rows || (k > 0 && row_of_slot[k] <= row_of_slot[k - 1])) return MIDAS_SNPS_ERR_INVALID_ARG;
  TableWriter w(path);
  if (!w.f) { gm_fail(err1024, path, 0, "cannot be written"); return MIDAS_SNPS_ERR_INVALID_ARG; }
  w.buf += "gene_id\tcount_case\tcount_control\teffect\tp_value\tq_value";
  if (n_perms > 0) w.buf += "\texceed\tp_perm\tq_perm";
  w.buf.push_back('\n');
  // (the slots ascend by row: one walk over the body finds every gene id)
  const char* s = m->base + m->body;
  const size_t n = m->size - m->body;
  size_t at = 0;
  int64_t row = 0;
  for (int64_t k = 0; k < n_slots; ++k) {
    for (; row < row_of_slot[k]; ++row) {
      const char* x = static_cast<const char*>(memchr(s + at, '\n', n - at));
      at = x ? (size_t)(x - s) + 1 : n;
    }
    size_t len = 0;
    while (at + len < n && s[at + len] != '\t' && s[at + len] != '\n') ++len;
    while (len > 0 && s[at + len - 1] == '\r') --len;
    w.buf.append(s + at, len);
    w.buf.push_back('\t');
    w.i64(count_case[k]);
    w.buf.push_back('\t');
    w.i64((int64_t)count[k] - count_case[k]);
    const double f[3] = {effect[k], p_value[k], q_value[k]};
    for (double v : f) { w.buf.push_back('\t'); w.f64(v); }
    if (n_perms > 0) {
      w.buf.push_back('\t');
      w.i64((int64_t)exceed[k]);
      w.buf.push_back('\t');
      w.f64(p_perm[k]);
      w.buf.push_back('\t');
      w.f64(q_perm[k]);
    }
    w.row_done();
  }
  if (!w.close()) { gm_fail(err1024, path, 0, "cannot be written"); return MIDAS_SNPS_ERR_INVALID_ARG; }
  return MIDAS_SNPS_OK;
}

}  // extern "C"
