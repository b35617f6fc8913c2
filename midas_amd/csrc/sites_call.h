// The site decisions of snp_diversity.py / call_consensus.py over a row group (sites_rows.h), for sites_scan.hip and
// sites_trees.hip:
//   site     one thread a row: GenomicSite.flag_samples, call_consensus, summary_stats, filter, in snps_summary.txt order.
//            The unweighted pooled frequency is numpy's pairwise add-reduce (blocks of 128, eight partial sums) over the
//            kept values, consumed in order; the weighted one is a left-to-right sum.  Where the reference raises instead
//            (round() of a frequency that is not finite, a weighted mean over depths that sum to 0) the site is reported, and
//            the earliest such row in file order ends the call as a malformed cell does
//   order    --max_sites: exclusive scan of the keep flags, a site stays while fewer than max_sites were kept before it
// SiteStep is the host side of the two: it owns their buffers, enqueues them for a group and answers what the group kept and
// which of its rows the reference reads.  Internal linkage, a copy in each including file; -ffp-contract=off (build.py): d*f
// rounds as the interpreter rounds it.
#pragma once
#include "sites_rows.h"

namespace midas {
namespace {

struct SiteP {
  const double* fv;            // [S][stride]
  const long long* dv;         // [S][stride]
  uint8_t* cell;               // [S][stride] bit 0: the sample is kept at the site
  const double* mean_depth;    // [S]
  const uint8_t* mask;         // [g] what the info table and the options decide (already offset to the group)
  long long g, stride;
  int S;
  long long site_depth;
  double site_ratio, allele_support, site_prev, site_maf;
  int weight, round_freq, mask_only;
  uint32_t* keep;              // [g] the site's keep decision
  double* pooled;              // [g]
  unsigned long long* err;     // min over (row << 32 | (sample + 1) << 3 | reason); nullptr: neither flag that can raise is set
};

// why a site's pooled frequency cannot be formed (the reference raises there): round() of a frequency that is not finite
// (MIDAS_SITES_ROUND), the weighted mean over kept samples whose depths sum to 0 (MIDAS_SITES_WEIGHT)
constexpr uint32_t kSiteNonFinite = 1, kSiteZeroDepth = 4;

// the kept frequencies of one site, in sample order
struct KeptIter {
  const double* fv;
  const uint8_t* cell;
  long long stride;
  int s, round_freq;
  __device__ double next() {
    while (!(cell[(long long)s * stride] & 1)) ++s;
    const double f = fv[(long long)s * stride];
    ++s;
    return round_freq ? rint(f) + 0.0 : f;      // (float(round(f)) is never -0.0)
  }
};

// numpy's pairwise_sum over n <= 128 values (eight partial sums, then the tail)
__device__ double pairwise_leaf(KeptIter& it, long long n) {
  if (n < 8) {
    double res = 0.0;
    for (long long i = 0; i < n; ++i) res += it.next();
    return res;
  }
  double r[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) r[j] = it.next();
  long long i = 8;
  for (; i < n - (n % 8); i += 8) {
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] += it.next();
  }
  double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
  for (; i < n; ++i) res += it.next();
  return res;
}

// numpy's add.reduce of n values: halves cut at multiples of eight down to blocks of at most 128, left before right
__device__ double pairwise_sum(KeptIter& it, long long n) {
  struct Frame { long long n; double left; int st; };
  Frame stk[40];
  int sp = 0;
  stk[sp++] = Frame{n, 0.0, 0};
  double ret = 0.0;
  while (sp > 0) {
    Frame& f = stk[sp - 1];
    long long n2 = f.n / 2;
    n2 -= n2 % 8;
    if (f.st == 0) {
      if (f.n <= 128) {
        ret = pairwise_leaf(it, f.n);
        --sp;
      } else {
        f.st = 1;
        stk[sp++] = Frame{n2, 0.0, 0};
      }
    } else if (f.st == 1) {
      f.left = ret;
      f.st = 2;
      stk[sp++] = Frame{f.n - n2, 0.0, 0};
    } else {
      ret = f.left + ret;
      --sp;
    }
  }
  return ret;
}

// compute_pooled_maf over the `count` kept samples of one site (fv, dv, cell point at the site's first cell): the weighted form
// is sum(d * f) / sum(d) left to right, the unweighted one numpy's mean.  *zero_depth: the weighted form has no value, the kept
// depths sum to 0.  The site kernel calls it, and so does the pass that resamples a site's reads (sites_resample.h).
__device__ double site_pooled(const double* fv, const long long* dv, const uint8_t* cell, long long stride, int S, long long count,
                              int weight, int round_freq, bool* zero_depth) {
  if (count == 0) return 0.0;
  if (!weight) {
    KeptIter it{fv, cell, stride, 0, round_freq};
    return __ddiv_rn(pairwise_sum(it, count), (double)count);
  }
  long long dsum = 0;
  double msum = 0.0;
  for (int s = 0; s < S; ++s) {
    const long long at = (long long)s * stride;
    if (!(cell[at] & 1)) continue;
    const double f = fv[at];
    const long long d = dv[at];
    dsum += d;
    msum += (double)d * (round_freq ? rint(f) + 0.0 : f);
  }
  if (dsum == 0) { *zero_depth = true; return 0.0; }
  return __ddiv_rn(msum, (double)dsum);
}

__global__ __launch_bounds__(256) void ss_site_kernel(SiteP p) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r >= p.g) return;
  long long count = 0;
  unsigned long long why = 0;                   // the first sample whose frequency round() refuses, kept or not
  for (int s = 0; s < p.S; ++s) {
    const long long at = (long long)s * p.stride + r;
    const long long d = p.dv[at];
    const double f = p.fv[at];
    if (p.round_freq && why == 0 && !isfinite(f)) why = ((unsigned long long)(s + 1) << 3) | kSiteNonFinite;
    bool keep = true;
    if (d < p.site_depth) keep = false;
    if (__ddiv_rn((double)d, p.mean_depth[s]) > p.site_ratio) keep = false;
    double m = f;                               // max(f, 1 - f) as Python's max: the first wins unless the second is greater
    if (1.0 - f > m) m = 1.0 - f;
    if (m < p.allele_support) keep = false;
    p.cell[at] = keep ? 1 : 0;
    if (keep) ++count;
  }
  bool zero_depth = false;
  const double pooled = site_pooled(p.fv + r, p.dv + r, p.cell + r, p.stride, p.S, count, p.weight, p.round_freq, &zero_depth);
  if (zero_depth && why == 0) why = kSiteZeroDepth;
  bool k = p.mask[r] != 0;
  if (!p.mask_only) {
    const double prev = __ddiv_rn((double)count, (double)p.S);
    if (p.site_prev != 0.0 && prev < (1e-6 > p.site_prev ? 1e-6 : p.site_prev)) k = false;
    if (p.site_maf != 0.0 && pooled < p.site_maf) k = false;
  }
  if (why != 0 && p.err) atomicMin(p.err, ((unsigned long long)r << 32) | why);
  p.keep[r] = k ? 1u : 0u;
  p.pooled[r] = pooled;
}

// keep[r] -> final: still below max_sites; rank[r] = kept sites of the group before r.  The row that fills max_sites is
// reported: the reference reads one more row after it and stops.
__global__ __launch_bounds__(256) void ss_order_kernel(const uint32_t* keep, const uint32_t* rank, long long g, long long kept_before,
                                                       long long max_sites, uint8_t* final_keep, long long* last_row) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r >= g) return;
  const long long pos = kept_before + rank[r];
  const bool k = keep[r] != 0 && (max_sites < 0 || pos < max_sites);
  final_keep[r] = k ? 1 : 0;
  if (k && max_sites >= 0 && pos == max_sites - 1) *last_row = r;
}

// a site whose pooled frequency cannot be formed (ss_site_kernel's err): its place in stats, the reason in words
int32_t site_pool_error(midas_snps_ctx* ctx, unsigned long long err, long long base, int64_t* stats) {
  const long long row = base + (long long)(err >> 32), slot = (long long)((err & 0xFFFFFFFFull) >> 3) - 1;
  const int why = (int)(err & 7u);
  stats[4] = 2 + why;
  stats[5] = row;
  stats[6] = slot;
  stats[0] = base;
  char buf[160];
  if (why == (int)kSiteNonFinite) snprintf(buf, sizeof buf, "data row %lld, sample %lld: the frequency to round is not a finite number", row, slot);
  else snprintf(buf, sizeof buf, "data row %lld: the depths of the kept samples sum to 0, so no depth-weighted frequency", row);
  return ss_fail(ctx, MIDAS_SNPS_ERR_BAD_LAYOUT, buf);
}

// The site kernel and the order of one row group after another.  run() enqueues them (events 3, 4, 5 bracket site and order)
// with the copies of what the host needs back; once the caller has synchronised, kept_g() ... pool_rows() hold for the group,
// check_rows() reports what the reference would raise on, and advance() moves on to the next group.
struct SiteStep {
  midas_snps_ctx* ctx;
  RowGroups& rg;
  const uint8_t* site_mask;      // [n_sites_max], the caller's
  long long max_sites;
  SiteP sp;                      // the options; mask and g are the group's
  uint8_t *d_cell = nullptr, *d_mask = nullptr, *d_final = nullptr;
  uint32_t *d_keep = nullptr, *d_rank = nullptr;
  double *d_pooled = nullptr, *d_mean = nullptr;
  long long* d_last = nullptr;
  unsigned long long* d_err = nullptr;
  long long kept = 0;            // sites retained in the groups before this one
  long long g = 0, last_row = -1;
  uint32_t last_keep = 0, last_rank = 0;
  unsigned long long err = kNoBad;

  SiteStep(midas_snps_ctx* c, RowGroups& r, const uint8_t* mask, long long site_depth, long long max_sites_in, const double* fparams5,
           int weight, int round_freq, int mask_only)
      : ctx(c), rg(r), site_mask(mask), max_sites(max_sites_in) {
    sp.site_depth = site_depth; sp.site_ratio = fparams5[0]; sp.allele_support = fparams5[1]; sp.site_prev = fparams5[2];
    sp.site_maf = fparams5[3]; sp.weight = weight; sp.round_freq = round_freq; sp.mask_only = mask_only;
  }

  // the buffers, once rg.init() has sized the groups.  with_err: the site kernel gets an error word (a caller that sets neither
  // MIDAS_SITES_ROUND nor MIDAS_SITES_WEIGHT needs none: nothing the reference raises on)
  int32_t init(const double* mean_depth, bool with_err) {
    const size_t G = (size_t)rg.G;
    if (with_err) SS_TRY(rg.dev.get(&d_err, 8));
    SS_TRY(rg.dev.get(&d_cell, rg.cells));
    SS_TRY(rg.dev.get(&d_mask, G));
    SS_TRY(rg.dev.get(&d_final, G));
    SS_TRY(rg.dev.get(&d_keep, G * 4));
    SS_TRY(rg.dev.get(&d_rank, G * 4));
    SS_TRY(rg.dev.get(&d_pooled, G * 8));
    SS_TRY(rg.dev.get(&d_mean, (size_t)rg.S * 8));
    SS_TRY(rg.dev.get(&d_last, 8));
    SS_TRY(hipMemcpyAsync(d_mean, mean_depth, (size_t)rg.S * 8, hipMemcpyHostToDevice, rg.st));
    sp.fv = rg.d_fv; sp.dv = rg.d_dv; sp.cell = d_cell; sp.mean_depth = d_mean; sp.mask = d_mask; sp.stride = rg.G; sp.S = rg.S;
    sp.keep = d_keep; sp.pooled = d_pooled;
    sp.err = d_err;
    return MIDAS_SNPS_OK;
  }

  // the group of g_in rows that rg.next() left
  int32_t run(long long g_in) {
    hipStream_t st = rg.st;
    g = g_in;
    sp.g = g;
    SS_TRY(hipMemcpyAsync(d_mask, site_mask + rg.base, (size_t)g, hipMemcpyHostToDevice, st));
    SS_TRY(hipEventRecord(rg.ev.e[3], st));
    if (d_err) SS_TRY(hipMemsetAsync(d_err, 0xFF, 8, st));
    hipLaunchKernelGGL(ss_site_kernel, dim3(nblocks(g, 256)), dim3(256), 0, st, sp);
    SS_TRY(hipGetLastError());
    SS_TRY(hipEventRecord(rg.ev.e[4], st));
    last_keep = last_rank = 0;
    last_row = -1;
    err = kNoBad;
    SS_TRY(hipMemsetAsync(d_last, 0xFF, 8, st));
    SS_TRY(launch_scan_u32(d_keep, d_rank, g, rg.d_scratch, st));
    hipLaunchKernelGGL(ss_order_kernel, dim3(nblocks(g, 256)), dim3(256), 0, st, d_keep, d_rank, g, kept, max_sites, d_final, d_last);
    SS_TRY(hipGetLastError());
    SS_TRY(hipEventRecord(rg.ev.e[5], st));
    SS_TRY(hipMemcpyAsync(&last_keep, d_keep + g - 1, 4, hipMemcpyDeviceToHost, st));
    SS_TRY(hipMemcpyAsync(&last_rank, d_rank + g - 1, 4, hipMemcpyDeviceToHost, st));
    SS_TRY(hipMemcpyAsync(&last_row, d_last, 8, hipMemcpyDeviceToHost, st));
    if (d_err) SS_TRY(hipMemcpyAsync(&err, d_err, 8, hipMemcpyDeviceToHost, st));
    return MIDAS_SNPS_OK;
  }

  // sites of the group that are retained
  long long kept_g() const {
    const long long n = (long long)last_rank + last_keep;
    return max_sites >= 0 ? std::min(n, max_sites - kept) : n;
  }
  // the rows the reference reads: all of the group, or up to the one after the row that fills max_sites -- whose cells it
  // converts, but whose pooled frequency it never forms
  long long read_rows() const { return last_row >= 0 ? last_row + 2 : g; }
  long long pool_rows() const { return max_sites == 0 ? 0 : last_row >= 0 ? last_row + 1 : g; }

  // a site that cannot be pooled or a row that cannot be read, among those rows: the error
  int32_t check_rows() {
    if (err != kNoBad && (long long)(err >> 32) < pool_rows() && call_error_comes_first(rg, read_rows(), err))
      return site_pool_error(ctx, err, rg.base, rg.stats);
    return rg.check_rows(read_rows());
  }

  // the group is done with; *stop: max_sites is filled.  Where its last row filled it, the row behind is still checked
  int32_t advance(bool* stop) {
    kept += kept_g();
    rg.advance(g);
    *stop = last_row >= 0;
    return last_row == g - 1 ? rg.check_row_behind() : MIDAS_SNPS_OK;
  }
};

}  // namespace
}  // namespace midas
