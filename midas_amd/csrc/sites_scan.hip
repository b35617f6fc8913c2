// snp_diversity.py / call_consensus.py on MI355X: the per-site loop of midas/analyze/parse_snps.py and of the
// two scripts over it, for all rows of snps_freq.txt / snps_depth.txt at once.  The matrices arrive as TEXT; parsing them is
// most of the work, so it happens here.
//
//   chunks   a run of bytes of each matrix is uploaded; its complete rows are the group's candidates
//   index    newlines counted per 16 bytes, the library's exclusive scan (device_sort.hip), newline k's position -> ends[k]
//   parse    one thread a row walks its fields; a cell of a selected sample is converted on the spot when it has the shape
//            [+-]digits[.digits][e[+-]digits] with a mantissa below 2^53 and a power of ten within +-22 (one exact
//            int -> fp64 conversion, one IEEE multiply or divide: correctly rounded), or [+-]digits up to 18 of them for
//            the depth; every other cell goes to a side list, which the host converts with its exact parser and patches
//            in before the site kernel runs.  Values land sample-major, [sample][row]
//   site     one thread a row: GenomicSite.flag_samples, call_consensus, summary_stats, filter, in snps_summary.txt order.
//            The unweighted pooled frequency is numpy's pairwise add-reduce (blocks of 128, eight partial sums) over the
//            kept values, consumed in order; the weighted one is a left-to-right sum.  Where the reference raises instead
//            (round() of a frequency that is not finite, a weighted mean over depths that sum to 0) the site is reported, and
//            the earliest such row in file order ends the call as a malformed cell does
//   order    --max_sites: exclusive scan of the keep flags, a site stays while fewer than max_sites were kept before it
//   sums     one wave a chain (a sample, or the pool): 64 rows loaded coalesced, then folded in lane order -- the fp64 sum
//            is the sequential one, bit for bit; per-gene chains switch accumulators where the gene index changes.
//            Accumulators live in device memory and carry from group to group
//   seq      call_consensus.py: one byte per (retained site, sample), sample-major
// (chunks, the line index and the pair kernel live in text_rows.h, shared with genes_compare.hip)
// strain_tracking.py (midas/analyze/track_strains.py) walks the same rows (RowGroups: chunks, index, parse, side lists):
//   mark     id_markers: one thread a row counts the samples that have the minor, the major, both alleles and any read
//            (x >= min_freq and round(x * depth) >= min_reads), folds them onto A, T, C, G and decides the marker; the scan
//            compacts the marker rows
//   bits     track_markers: the matched sites of a group (one byte a site from the host: none, major, minor) are ranked by the
//            scan; one wave calls 64 of them for one sample, its ballot is a word of the bit matrix [sample][word]
//   pairs    both[i][j] += popcount(B[i][w] & B[j][w]) in 64 x 64 tiles of sample pairs staged through LDS; integer sums, held
//            on the device across groups
// snp_trees.py walks them once more (midas_sites_consensus_pairs): the site kernel and the order of call_consensus.py, then
//   planes   the consensus calls of a group's retained sites as two bit matrices, `called` and `minor`, one wave a word
//   pairs    both[i][j] += popcount(C_i & C_j), diff[i][j] += popcount(C_i & C_j & (M_i ^ M_j)), the tiling of the pair kernel
// This file is compiled with -ffp-contract=off (build.py): 2*f*(1-f), d*f and x*depth round as the interpreter rounds them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <string>
#include <string_view>
#include <vector>

#include "../../include/midas_snps.h"
#include "ctx_internal.h"
#include "kernels.h"
#include "text_numbers.h"
#include "text_rows.h"

namespace midas {
namespace {

// float(cell) for [+-]digits[.digits][e[+-]digits], mantissa < 2^53, |power of ten| <= 22: exact by construction
__device__ bool fast_f64(const char* s, int n, double* out) {
  static const double p10[23] = {1e0,  1e1,  1e2,  1e3,  1e4,  1e5,  1e6,  1e7,  1e8,  1e9,  1e10, 1e11,
                                 1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};
  if (n <= 0) return false;
  int i = 0;
  bool neg = false;
  if (s[0] == '+' || s[0] == '-') { neg = s[0] == '-'; i = 1; }
  unsigned long long m = 0;
  constexpr unsigned long long lim = (1ull << 53) - 1;
  int nd = 0, nfrac = 0;
  for (; i < n && is_digit(s[i]); ++i, ++nd) {
    const unsigned d = (unsigned)(s[i] - '0');
    if (m > (lim - d) / 10) return false;
    m = m * 10 + d;
  }
  if (nd == 0) return false;
  if (i < n && s[i] == '.') {
    for (++i; i < n && is_digit(s[i]); ++i, ++nfrac) {
      const unsigned d = (unsigned)(s[i] - '0');
      if (m > (lim - d) / 10) return false;
      m = m * 10 + d;
    }
    if (nfrac == 0) return false;
  }
  int ex = 0;
  if (i < n && (s[i] == 'e' || s[i] == 'E')) {
    ++i;
    bool eneg = false;
    if (i < n && (s[i] == '+' || s[i] == '-')) { eneg = s[i] == '-'; ++i; }
    int ne = 0;
    for (; i < n && is_digit(s[i]); ++i, ++ne) {
      if (ne == 3) return false;
      ex = ex * 10 + (s[i] - '0');
    }
    if (ne == 0) return false;
    if (eneg) ex = -ex;
  }
  if (i != n) return false;
  double x = (double)(long long)m;
  if (m != 0) {
    const int e10 = ex - nfrac;
    if (e10 < -22 || e10 > 22) return false;
    x = e10 < 0 ? __ddiv_rn(x, p10[-e10]) : __dmul_rn(x, p10[e10]);
  }
  *out = neg ? -x : x;
  return true;
}

// int(cell) for [+-]digits, at most 18 digits
__device__ bool fast_i64(const char* s, int n, long long* out) {
  if (n <= 0) return false;
  int i = 0;
  bool neg = false;
  if (s[0] == '+' || s[0] == '-') { neg = s[0] == '-'; i = 1; }
  if (i == n || n - i > 18) return false;
  long long m = 0;
  for (; i < n; ++i) {
    if (!is_digit(s[i])) return false;
    m = m * 10 + (s[i] - '0');
  }
  *out = neg ? -m : m;
  return true;
}

struct ParseP {
  const char* text;            // the chunk
  const uint32_t* ends;        // newline offsets of its rows
  long long g, stride;         // rows to parse; row stride of a sample's values
  const int32_t* col_slot;     // [n_cols] matrix column -> selected sample, or -1
  int n_cols;                  // columns a row must have (1 + the largest selected column)
  void* val;                   // [n_samples][stride] f64 or i64
  SideCell* side;
  uint32_t* side_n;
  uint32_t side_cap;
  unsigned long long* bad;     // min over (row << 32 | slot + 1); slot + 1 == 0: the row is short
};

template <bool kInt>
__global__ __launch_bounds__(256) void ss_parse_kernel(ParseP p) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r >= p.g) return;
  const uint32_t b = r == 0 ? 0u : p.ends[r - 1] + 1u;
  uint32_t e = p.ends[r];
  const char* t = p.text;
  if (e > b && t[e - 1] == '\r') --e;
  uint32_t q = b;
  while (q < e && t[q] != '\t') ++q;         // the site id
  for (int c = 0; c < p.n_cols; ++c) {
    if (q >= e) {                            // no tab left: the row lacks column c
      atomicMin(p.bad, (unsigned long long)r << 32);
      return;
    }
    const uint32_t fs = ++q;
    while (q < e && t[q] != '\t') ++q;
    const int slot = p.col_slot[c];
    if (slot < 0) continue;
    const int len = (int)(q - fs);
    const long long at = (long long)slot * p.stride + r;
    bool ok;
    if (kInt) {
      long long v = 0;
      ok = fast_i64(t + fs, len, &v);
      static_cast<long long*>(p.val)[at] = v;
    } else {
      double v = 0.0;
      ok = fast_f64(t + fs, len, &v);
      static_cast<double*>(p.val)[at] = v;
    }
    if (!ok) {
      const uint32_t k = atomicAdd(p.side_n, 1u);
      if (k < p.side_cap) p.side[k] = SideCell{(uint32_t)r, (uint32_t)slot, fs, (uint32_t)len};
    }
  }
}

template <class T>
__global__ __launch_bounds__(256) void ss_patch_kernel(T* val, const long long* at, const T* v, long long n) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) val[at[i]] = v[i];
}

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

__global__ __launch_bounds__(256) void ss_site_kernel(SiteP p) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r >= p.g) return;
  long long count = 0, dsum = 0;
  double msum = 0.0;
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
    if (keep) {
      ++count;
      if (p.weight) {
        const double f2 = p.round_freq ? rint(f) + 0.0 : f;
        dsum += d;
        msum += (double)d * f2;
      }
    }
  }
  double pooled = 0.0;
  if (count > 0) {
    if (p.weight) {
      if (dsum == 0) { if (why == 0) why = kSiteZeroDepth; }
      else pooled = __ddiv_rn(msum, (double)dsum);
    } else {
      KeptIter it{p.fv + r, p.cell + r, p.stride, 0, p.round_freq};
      pooled = __ddiv_rn(pairwise_sum(it, count), (double)count);
    }
  }
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

struct SumP {
  const double* fv;            // [S][stride], or the pooled frequency [g] (pooled != 0)
  const long long* dv;
  const uint8_t* cell;
  const uint8_t* final_keep;   // [g]
  const int32_t* gene;         // [g] (already offset), per_gene only
  long long g, stride;
  int pooled, per_gene, round_freq;
  long long n_genes;           // accumulators per chain (1 genome-wide)
  double snp_maf;
  double* pi;                  // [chains][n_genes]
  long long* snps;
  long long* sites;
  long long* depth;
  unsigned long long* no_gene; // kept sites without a gene id in a per-gene run
};

// one wave per chain
__global__ __launch_bounds__(64) void ss_sums_kernel(SumP p) {
  const int chain = blockIdx.x, lane = threadIdx.x;
  const long long base = (long long)chain * p.n_genes;
  long long cur = p.per_gene ? -1 : 0;
  double pi = 0.0;
  long long snps = 0, sites = 0, depth = 0;
  if (!p.per_gene) { pi = p.pi[base]; snps = p.snps[base]; sites = p.sites[base]; depth = p.depth[base]; }
  for (long long r0 = 0; r0 < p.g; r0 += 64) {
    const long long r = r0 + lane;
    bool on = false;
    double term = 0.0;
    long long d = 0;
    int snp = 0, gi = -1;
    if (r < p.g && p.final_keep[r]) {
      const long long at = (long long)chain * p.stride + r;
      on = p.pooled ? true : (p.cell[at] & 1) != 0;
      if (on) {
        double f = p.pooled ? p.fv[r] : p.fv[at];
        if (!p.pooled && p.round_freq) f = rint(f) + 0.0;
        term = (2.0 * f) * (1.0 - f);
        double m = f;                           // min(f, 1 - f) as Python's min
        if (1.0 - f < m) m = 1.0 - f;
        snp = m >= p.snp_maf ? 1 : 0;
        d = p.pooled ? 0 : p.dv[at];
        if (p.per_gene) gi = p.gene[r];
      }
    }
    if (p.per_gene && chain == 0) {             // kept sites without a gene id, whichever samples are kept there
      const unsigned long long lost = __ballot(r < p.g && p.final_keep[r] && p.gene[r] < 0);
      if (lane == 0 && lost) atomicAdd(p.no_gene, (unsigned long long)__popcll((long long)lost));
    }
    unsigned long long live = __ballot(on);
    const int tlo = __double2loint(term), thi = __double2hiint(term);
    while (live) {
      const int k = __ffsll((long long)live) - 1;
      live &= live - 1;
      const double t = __hiloint2double(__builtin_amdgcn_readlane(thi, k), __builtin_amdgcn_readlane(tlo, k));
      if (p.per_gene) {
        const long long gk = __builtin_amdgcn_readlane(gi, k);
        if (gk != cur) {
          if (cur >= 0 && lane == 0) { p.pi[base + cur] = pi; p.snps[base + cur] = snps; p.sites[base + cur] = sites; p.depth[base + cur] = depth; }
          cur = gk;
          if (cur >= 0) { pi = p.pi[base + cur]; snps = p.snps[base + cur]; sites = p.sites[base + cur]; depth = p.depth[base + cur]; }
        }
        if (cur < 0) continue;
      }
      pi += t;
      snps += __builtin_amdgcn_readlane(snp, k);
      sites += 1;
      const unsigned dlo = (unsigned)__builtin_amdgcn_readlane((int)(d & 0xFFFFFFFFll), k);
      const unsigned dhi = (unsigned)__builtin_amdgcn_readlane((int)(d >> 32), k);
      depth += (long long)(((unsigned long long)dhi << 32) | dlo);
    }
  }
  if (cur >= 0 && lane == 0) { p.pi[base + cur] = pi; p.snps[base + cur] = snps; p.sites[base + cur] = sites; p.depth[base + cur] = depth; }
}

// fetch_consensus for the retained sites of the group: seq[s][rank] (rank among the group's retained sites)
__global__ __launch_bounds__(256) void ss_seq_kernel(const double* fv, const long long* dv, const uint8_t* cell, const uint8_t* final_keep,
                                                     const uint32_t* rank, const char* minor, const char* major, long long g, long long stride,
                                                     int S, uint8_t* seq) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r >= g || !final_keep[r]) return;
  const long long pos = rank[r];
  const char mi = minor[r], ma = major[r];
  for (int s = 0; s < S; ++s) {
    const long long at = (long long)s * stride + r;
    char c = '-';
    if ((cell[at] & 1) && dv[at] != 0) c = fv[at] >= 0.5 ? mi : ma;
    seq[(long long)s * stride + pos] = (uint8_t)c;
  }
}


// ---- strain_tracking.py: marker alleles and their sharing between samples -----------------------------------------------------
// A cell's call (midas/analyze/track_strains.py): the allele with frequency x is present in a sample with depth d != 0 when
// x >= min_freq and round(x * d) >= min_reads; round() is half to even on the fp64 product: rint.
constexpr uint32_t kCallNonFinite = 1, kCallMinorLetter = 2, kCallMajorLetter = 3;      // why a site cannot be called

struct MarkP {
  const double* fv;            // [S][stride]
  const long long* dv;
  const uint8_t* minor;        // [g] 0..3 = A, T, C, G; anything else: another string
  const uint8_t* major;
  long long g, stride;         // rows to call
  int S;
  double min_freq, min_reads;
  long long allele_prev;
  uint32_t* flag;              // [g] the site is a marker
  int32_t* row6;               // [g][6] allele, total, count A, T, C, G
  unsigned long long* err;     // min over (row << 32 | sample << 2 | reason)
};

// id_markers: count_alleles over the samples in order, then the marker decision
__global__ __launch_bounds__(256) void ss_mark_kernel(MarkP p) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r >= p.g) return;
  const int mi = p.minor[r], ma = p.major[r];
  int n_minor = 0, n_major = 0, n_both = 0, total = 0;
  uint32_t why = 0;
  int s = 0;
  for (; s < p.S; ++s) {
    const long long at = (long long)s * p.stride + r;
    const long long d = p.dv[at];
    if (d == 0) continue;
    const double f = p.fv[at];
    bool has_minor = false, has_major = false;
    if (f >= p.min_freq) {
      const double x = f * (double)d;
      if (!isfinite(x)) { why = kCallNonFinite; break; }
      if (rint(x) >= p.min_reads) {
        if (mi > 3) { why = kCallMinorLetter; break; }
        has_minor = true;
      }
    }
    const double q = 1.0 - f;
    if (q >= p.min_freq) {
      const double x = q * (double)d;
      if (!isfinite(x)) { why = kCallNonFinite; break; }
      if (rint(x) >= p.min_reads) {
        if (ma > 3) { why = kCallMajorLetter; break; }
        has_major = true;
      }
    }
    n_minor += has_minor;
    n_major += has_major;
    n_both += has_minor && has_major;
    ++total;
  }
  if (why) {
    atomicMin(p.err, ((unsigned long long)r << 32) | ((unsigned long long)s << 2) | why);
    p.flag[r] = 0;
    return;
  }
  int c[4] = {0, 0, 0, 0};       // sets of samples by letter: a sample that has both counts once where the letters agree
  if (mi <= 3) c[mi] += n_minor;
  if (ma <= 3) c[ma] += n_major;
  if (mi == ma && mi <= 3) c[mi] -= n_both;
  int letters = 0, rare = -1;    // the smaller of two counts; a tie goes to the earlier of A, T, C, G (a stable sort)
  for (int k = 0; k < 4; ++k) {
    if (c[k] <= 0) continue;
    ++letters;
    if (rare < 0 || c[k] < c[rare]) rare = k;
  }
  const bool marker = letters == 2 && (long long)c[rare] <= p.allele_prev;
  p.flag[r] = marker ? 1u : 0u;
  int32_t* o = p.row6 + 6 * r;
  o[0] = rare; o[1] = total; o[2] = c[0]; o[3] = c[1]; o[4] = c[2]; o[5] = c[3];
}

// the markers of the group, in row order: out[rank] = row, allele, total, counts
__global__ __launch_bounds__(256) void ss_mark_compact_kernel(const uint32_t* flag, const uint32_t* rank, const int32_t* row6, long long g,
                                                              long long base, int32_t* out7) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r >= g || !flag[r]) return;
  int32_t* o = out7 + 7 * (long long)rank[r];
  o[0] = (int32_t)(base + r);
#pragma unroll
  for (int k = 0; k < 6; ++k) o[1 + k] = row6[6 * r + k];
}

__global__ __launch_bounds__(256) void ss_which_flag_kernel(const uint8_t* which, long long g, uint32_t* flag) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r < g) flag[r] = which[r] != 0 ? 1u : 0u;
}

// matched site k of the group -> its row and its allele (1 major, 2 minor): row << 2 | which
__global__ __launch_bounds__(256) void ss_which_list_kernel(const uint8_t* which, const uint32_t* rank, long long g, uint32_t* list) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r < g && which[r] != 0) list[rank[r]] = ((uint32_t)r << 2) | which[r];
}

// track_markers: the bit matrix.  One wave a (sample, 64 matched sites): a lane calls its site, the ballot is the word.
__global__ __launch_bounds__(256) void ss_bits_kernel(const double* fv, const long long* dv, const uint32_t* list, long long m, long long stride,
                                                      int S, double min_freq, double min_reads, unsigned long long* bits, long long wstride,
                                                      unsigned long long* err) {
  const int s = blockIdx.y * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (s >= S) return;                                  // (the whole wave)
  const long long k = (long long)blockIdx.x * 64 + lane;
  bool present = false;
  if (k < m) {
    const uint32_t e = list[k];
    const long long r = e >> 2;
    const long long at = (long long)s * stride + r;
    const long long d = dv[at];
    if (d != 0) {
      const double f = fv[at];
      const double mf = (e & 3u) == 1u ? 1.0 - f : f;
      const double x = mf * (double)d;
      if (!isfinite(x)) atomicMin(err, ((unsigned long long)r << 32) | ((unsigned long long)s << 2) | kCallNonFinite);
      else present = mf >= min_freq && rint(x) >= min_reads;
    }
  }
  const unsigned long long word = __ballot(present);
  if (lane == 0) bits[(long long)s * wstride + blockIdx.x] = word;
}

// ---- snp_trees.py: the consensus calls as two bit planes, and their pair counts -------------------------------------------------
// retained site k of the group (rank among final_keep) -> its row
__global__ __launch_bounds__(256) void ss_keep_list_kernel(const uint8_t* final_keep, const uint32_t* rank, long long g, uint32_t* list) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r < g && final_keep[r]) list[rank[r]] = (uint32_t)r;
}

// The planes [sample][64 retained sites a word], from the parsed cells.  One wave a (sample, 64 retained sites): `called` where
// ss_seq_kernel writes a letter (the cell is kept and depth != 0), `minor` where that letter is the minor allele (freq >= 0.5).
__global__ __launch_bounds__(256) void ss_planes_kernel(const double* fv, const long long* dv, const uint8_t* cell, const uint32_t* list,
                                                        long long m, long long stride, int S, unsigned long long* called,
                                                        unsigned long long* minor, long long wstride) {
  const int s = blockIdx.y * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (s >= S) return;                                  // (the whole wave)
  const long long k = (long long)blockIdx.x * 64 + lane;
  bool is_called = false, is_minor = false;
  if (k < m) {
    const long long at = (long long)s * stride + list[k];
    if ((cell[at] & 1) && dv[at] != 0) {
      is_called = true;
      is_minor = fv[at] >= 0.5;
    }
  }
  const unsigned long long wc = __ballot(is_called), wm = __ballot(is_minor);
  if (lane == 0) {
    called[(long long)s * wstride + blockIdx.x] = wc;
    minor[(long long)s * wstride + blockIdx.x] = wm;
  }
}

// both[i][j] += popcount(C_i & C_j), diff[i][j] += popcount(C_i & C_j & (M_i ^ M_j)) for i <= j: ss_pairs_kernel's tiling (a
// 64 x 64 tile of pairs a workgroup, a 4 x 4 part of it a thread, a run of words along blockIdx.y) over two planes.  Four strips
// are staged, 16 words at a time: the static LDS of ss_pairs_kernel's two strips of 32.
constexpr int kPlaneRun = kPairRun / 2;
__global__ __launch_bounds__(256) void ss_plane_pairs_kernel(const unsigned long long* called, const unsigned long long* minor,
                                                             long long wstride, long long n_words, long long run_words, int S,
                                                             int tiles_side, unsigned long long* both, unsigned long long* diff) {
  __shared__ unsigned long long ca[kPlaneRun][kPairPad], cb[kPlaneRun][kPairPad], ma[kPlaneRun][kPairPad], mb[kPlaneRun][kPairPad];
  int ti = 0, left = blockIdx.x;
  while (left >= tiles_side - ti) { left -= tiles_side - ti; ++ti; }
  const int tj = ti + left;
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

// The rows of the two matrices on the device, a group at a time: upload, line index, cell parse, side-list patching.  Every
// entry point of this file walks the tables through it: next() leaves the group's cells in d_fv / d_dv, [sample][G].
struct RowGroups {
  midas_snps_ctx* ctx;
  hipStream_t st;
  SsBufs& dev;
  SsEvents& ev;                  // e[1], e[2], e[3] are used here
  float* ms;                     // [0] upload + index (host clock), [1] index, [2] parse
  int64_t* stats;                // the caller's out_stats16: [2] / [3] cells converted by the host, [0], [4..6] on a bad row
  int S = 0, n_cols = 0;
  long long G = 0, chunk_bytes = 0, n_sites_max = 0;
  size_t cells = 0;
  Chunk ck[2];
  uint32_t* d_scratch = nullptr;
  double* d_fv = nullptr;
  long long* d_dv = nullptr;
  int32_t* d_col_slot = nullptr;
  long long* d_patch_at = nullptr;
  void* d_patch_v = nullptr;
  size_t patch_cap = 0;
  std::vector<SideCell> side_h;
  std::vector<long long> patch_at;
  std::vector<double> patch_f;
  std::vector<long long> patch_i;
  long long base = 0, groups = 0;
  uint32_t end_at[2] = {0, 0};
  unsigned long long bad[2] = {kNoBad, kNoBad};

  static constexpr long long kChunkMax = (1ll << 30);       // newline offsets are 32-bit

  RowGroups(midas_snps_ctx* c, SsBufs& d, SsEvents& e, float* ms8, int64_t* stats16) : ctx(c), st(c->stream), dev(d), ev(e), ms(ms8), stats(stats16) {}

  int32_t alloc_chunk(Chunk& c, long long cb) { return chunk_alloc(ctx, dev, c, cb); }

  // sizes: rows a group (G) and bytes a chunk, from the caller or from a quarter of the free device memory; per_row = the
  // device bytes a row of the group takes in the caller's and in these buffers
  int32_t init(const char* freq, long long freq_bytes, const char* depth, long long depth_bytes, long long n_max, int n_samples,
               const std::vector<int32_t>& col_slot, long long G_in, long long chunk_in, long long per_row) {
    S = n_samples;
    n_cols = (int)col_slot.size();
    n_sites_max = n_max;
    G = G_in;
    chunk_bytes = chunk_in;
    if (G == 0 || chunk_bytes == 0) {
      size_t free_b = 0, total_b = 0;
      SS_TRY(hipMemGetInfo(&free_b, &total_b));
      const long long budget = (long long)(free_b / 4);
      if (chunk_bytes == 0) chunk_bytes = std::min<long long>(kChunkMax, std::max<long long>(1 << 20, budget / 8));
      if (G == 0) G = std::max<long long>(1, (budget - std::min(budget / 2, 5 * chunk_bytes / 2)) / per_row);
    }
    chunk_bytes = std::min(std::max<long long>(chunk_bytes, 64), kChunkMax);
    chunk_bytes = std::min(chunk_bytes, std::max<long long>(64, std::max(freq_bytes, depth_bytes) + 1));
    G = std::min<long long>(std::min<long long>(G, n_sites_max), chunk_bytes);
    G = std::max<long long>(G, 1);
    cells = (size_t)G * (size_t)S;
    if (cells > 0xFFFFFFF0ull) return ss_fail(ctx, MIDAS_SNPS_ERR_UNSUPPORTED, "a row group beyond 2^32 cells: lower group_rows");
    for (auto& x : ev.e) SS_TRY(hipEventCreate(&x));
    ck[0].host = freq; ck[0].bytes = freq_bytes;
    ck[1].host = depth; ck[1].bytes = depth_bytes;
    for (Chunk& c : ck) {
      int32_t rc = alloc_chunk(c, chunk_bytes);
      if (rc != MIDAS_SNPS_OK) return rc;
      SS_TRY(dev.get(&c.d_ends, ((size_t)G + 1) * 4));
      SS_TRY(dev.get(&c.d_side, cells * sizeof(SideCell)));
      SS_TRY(dev.get(&c.d_side_n, 4));
      SS_TRY(dev.get(&c.d_bad, 8));
    }
    SS_TRY(dev.get(&d_scratch, std::max(scan_scratch_words((kChunkMax + 16) / 16), scan_scratch_words(G)) * 4));
    SS_TRY(dev.get(&d_fv, cells * 8));
    SS_TRY(dev.get(&d_dv, cells * 8));
    SS_TRY(dev.get(&d_col_slot, (size_t)n_cols * 4));
    SS_TRY(hipMemcpyAsync(d_col_slot, col_slot.data(), (size_t)n_cols * 4, hipMemcpyHostToDevice, st));
    SS_TRY(hipStreamSynchronize(st));          // (col_slot is the caller's)
    return MIDAS_SNPS_OK;
  }

  hipError_t lap(int a, int b, int slot) {
    float t = 0.f;
    const hipError_t e = hipEventElapsedTime(&t, ev.e[a], ev.e[b]);
    if (e == hipSuccess) ms[slot] += t;
    return e;
  }

  // upload the next chunk of one matrix and index its lines (text_rows.h)
  int32_t load_chunk(Chunk& c) { return chunk_load(ctx, st, ev, c, chunk_bytes, G, d_scratch, &ms[1]); }

  // the next group: *g_out complete rows of both matrices parsed into d_fv / d_dv, or 0 when the rows are used up
  int32_t next(long long* g_out) {
    *g_out = 0;
    while (base < n_sites_max) {
      // ---- the group's rows: complete lines of both chunks ----------------------------------------------------------------
      const auto t_load = std::chrono::steady_clock::now();
      for (Chunk& c : ck) {
        int32_t rc = load_chunk(c);
        if (rc != MIDAS_SNPS_OK) return rc;
      }
      // (host clock around copies that end in a synchronise: upload + index of both chunks; the index alone is ms[1])
      ms[0] += std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_load).count();
      const long long g = std::min(std::min(ck[0].lines, ck[1].lines), std::min(G, n_sites_max - base));
      if (g == 0) {
        bool grow = false;
        for (Chunk& c : ck)
          if (c.lines == 0 && !c.at_eof) grow = true;
        if (!grow) return MIDAS_SNPS_OK;     // one of the matrices has no row left: the reference stops here too
        if (chunk_bytes >= kChunkMax) return ss_fail(ctx, MIDAS_SNPS_ERR_UNSUPPORTED, "a matrix row longer than 1 GiB");
        chunk_bytes = std::min(kChunkMax, chunk_bytes * 2);
        for (Chunk& c : ck) {
          int32_t rc = alloc_chunk(c, chunk_bytes);
          if (rc != MIDAS_SNPS_OK) return rc;
        }
        continue;
      }
      ++groups;
      // ---- parse ---------------------------------------------------------------------------------------------------------
      SS_TRY(hipEventRecord(ev.e[2], st));
      for (int m = 0; m < 2; ++m) {
        Chunk& c = ck[m];
        SS_TRY(hipMemsetAsync(c.d_side_n, 0, 4, st));
        SS_TRY(hipMemsetAsync(c.d_bad, 0xFF, 8, st));
        ParseP pp;
        pp.text = c.d_text; pp.ends = c.d_ends; pp.g = g; pp.stride = G; pp.col_slot = d_col_slot; pp.n_cols = n_cols;
        pp.val = m == 0 ? (void*)d_fv : (void*)d_dv; pp.side = c.d_side; pp.side_n = c.d_side_n; pp.side_cap = (uint32_t)cells;
        pp.bad = c.d_bad;
        if (m == 0) hipLaunchKernelGGL(ss_parse_kernel<false>, dim3(nblocks(g, 256)), dim3(256), 0, st, pp);
        else hipLaunchKernelGGL(ss_parse_kernel<true>, dim3(nblocks(g, 256)), dim3(256), 0, st, pp);
        SS_TRY(hipGetLastError());
      }
      SS_TRY(hipEventRecord(ev.e[3], st));
      uint32_t side_n[2] = {0, 0};
      end_at[0] = end_at[1] = 0;
      bad[0] = bad[1] = kNoBad;
      for (int m = 0; m < 2; ++m) {
        SS_TRY(hipMemcpyAsync(&side_n[m], ck[m].d_side_n, 4, hipMemcpyDeviceToHost, st));
        SS_TRY(hipMemcpyAsync(&bad[m], ck[m].d_bad, 8, hipMemcpyDeviceToHost, st));
        SS_TRY(hipMemcpyAsync(&end_at[m], ck[m].d_ends + g - 1, 4, hipMemcpyDeviceToHost, st));
      }
      SS_TRY(hipStreamSynchronize(st));
      SS_TRY(lap(2, 3, 2));
      // ---- the side lists: cells off the fast path, converted by the host's exact parser and patched in ----------------------
      for (int m = 0; m < 2; ++m) {
        const uint32_t n = side_n[m];
        stats[2 + m] += n;
        if (n == 0) continue;
        side_h.resize(n);
        SS_TRY(hipMemcpy(side_h.data(), ck[m].d_side, (size_t)n * sizeof(SideCell), hipMemcpyDeviceToHost));
        patch_at.clear(); patch_f.clear(); patch_i.clear();
        const char* text = ck[m].host + ck[m].at;
        for (const SideCell& sc : side_h) {
          // (a cell that starts at the appended terminator of an unterminated last line is empty: off + len stays inside)
          const std::string_view cell(text + sc.off, sc.len);
          bool ok;
          double vf = 0.0;
          int64_t vi = 0;
          if (m == 0) ok = parse_f64_py(cell, &vf);
          else ok = parse_i64_py(cell, &vi);
          if (!ok) {
            bad[m] = std::min(bad[m], ((unsigned long long)sc.row << 32) | (sc.slot + 1ull));
            continue;
          }
          patch_at.push_back((long long)sc.slot * G + sc.row);
          if (m == 0) patch_f.push_back(vf); else patch_i.push_back((long long)vi);
        }
        const size_t np = patch_at.size();
        if (np == 0) continue;
        if (np > patch_cap) {
          patch_cap = std::max(np, patch_cap * 2);
          SS_TRY(dev.get(&d_patch_at, patch_cap * 8));
          SS_TRY(dev.get((char**)&d_patch_v, patch_cap * 8));
        }
        SS_TRY(hipMemcpyAsync(d_patch_at, patch_at.data(), np * 8, hipMemcpyHostToDevice, st));
        SS_TRY(hipMemcpyAsync(d_patch_v, m == 0 ? (const void*)patch_f.data() : (const void*)patch_i.data(), np * 8, hipMemcpyHostToDevice, st));
        if (m == 0) hipLaunchKernelGGL(ss_patch_kernel<double>, dim3(nblocks((long long)np, 256)), dim3(256), 0, st, d_fv, d_patch_at, (const double*)d_patch_v, (long long)np);
        else hipLaunchKernelGGL(ss_patch_kernel<long long>, dim3(nblocks((long long)np, 256)), dim3(256), 0, st, d_dv, d_patch_at, (const long long*)d_patch_v, (long long)np);
        SS_TRY(hipGetLastError());
        SS_TRY(hipStreamSynchronize(st));       // (the host vectors are reused by the other matrix)
      }
      *g_out = g;
      return MIDAS_SNPS_OK;
    }
    return MIDAS_SNPS_OK;
  }

  // a short row or a cell that is no number among the first read_rows rows of the group: the error, with its place in stats
  int32_t check_rows(long long read_rows) {
    static const char* kFile[2] = {"freq", "depth"};
    // (the reference converts row by row, sample by sample, the frequency before the depth: the smaller key first)
    for (int m = bad[1] < bad[0] ? 1 : 0, k = 0; k < 2; ++k, m ^= 1) {
      if (bad[m] == kNoBad || (long long)(bad[m] >> 32) >= read_rows) continue;
      const long long row = base + (long long)(bad[m] >> 32);
      const long long slot = (long long)(bad[m] & 0xFFFFFFFFull) - 1;
      stats[4] = m + 1;
      stats[5] = row;
      stats[6] = slot;
      stats[0] = base;
      char buf[160];
      if (slot < 0) snprintf(buf, sizeof buf, "%s matrix, data row %lld: fewer than %d sample columns", kFile[m], row, n_cols);
      else snprintf(buf, sizeof buf, "%s matrix, data row %lld, sample %lld: not a number", kFile[m], row, slot);
      return ss_fail(ctx, MIDAS_SNPS_ERR_BAD_LAYOUT, buf);
    }
    return MIDAS_SNPS_OK;
  }

  // the first of the group's first read_rows rows that is short or holds a cell that is no number; -1: none
  long long first_bad_row(long long read_rows) const {
    long long row = -1;
    for (int m = 0; m < 2; ++m) {
      if (bad[m] == kNoBad || (long long)(bad[m] >> 32) >= read_rows) continue;
      if (row < 0 || (long long)(bad[m] >> 32) < row) row = (long long)(bad[m] >> 32);
    }
    return row;
  }

  // the group is done with: the next one starts behind its last row
  void advance(long long g) {
    base += g;
    for (int m = 0; m < 2; ++m) ck[m].at = std::min(ck[m].bytes, ck[m].at + (long long)end_at[m] + 1);
  }

  // max_sites was filled by the last row of the group just done with: the one row more that the reference converts (and then
  // stops at) opens the next group
  int32_t check_row_behind() {
    long long g = 0;
    const int32_t rc = next(&g);
    if (rc != MIDAS_SNPS_OK || g == 0) return rc;
    return check_rows(1);
  }
};

// The reference converts a row's cells and then calls the site, row by row: of a row that cannot be read and a site that
// cannot be called, the one it meets first is the error, whatever the row groups are (a row with both: the cells come first).
bool call_error_comes_first(const RowGroups& rg, long long g, unsigned long long err) {
  if (err == kNoBad) return false;
  const long long bad_row = rg.first_bad_row(g);
  return bad_row < 0 || (long long)(err >> 32) < bad_row;
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

}  // namespace
}  // namespace midas

using namespace midas;

extern "C" int32_t midas_sites_scan(midas_snps_ctx* ctx, const char* freq, int64_t freq_bytes, const char* depth, int64_t depth_bytes,
                                    int64_t n_sites_max, const uint8_t* site_mask, const int32_t* site_gene, const char* minor,
                                    const char* major, int32_t n_samples, const int32_t* sample_col, const double* mean_depth,
                                    const double* fparams5, const int64_t* iparams8, double* out_pi, int64_t* out_snps,
                                    int64_t* out_sites, int64_t* out_depth, uint8_t* out_seq, double* dump_freq, int64_t* dump_depth,
                                    uint8_t* dump_keep, double* dump_pooled, int64_t* out_stats16, float* out_ms8) {
  if (!ctx || freq_bytes < 0 || depth_bytes < 0 || (freq_bytes > 0 && !freq) || (depth_bytes > 0 && !depth) || n_sites_max < 0 ||
      n_samples < 1 || !sample_col || !mean_depth || !fparams5 || !iparams8 || !out_stats16 || (n_sites_max > 0 && !site_mask))
    return MIDAS_SNPS_ERR_INVALID_ARG;
  const long long site_depth = iparams8[0], max_sites = iparams8[1], flags = iparams8[2], seq_cap = iparams8[6];
  const long long n_genes_in = iparams8[3];
  const int weight = flags & MIDAS_SITES_WEIGHT ? 1 : 0, round_freq = flags & MIDAS_SITES_ROUND ? 1 : 0,
            pooled = flags & MIDAS_SITES_POOLED ? 1 : 0, per_gene = flags & MIDAS_SITES_PER_GENE ? 1 : 0,
            mask_only = flags & MIDAS_SITES_MASK_ONLY ? 1 : 0, want_seq = flags & MIDAS_SITES_SEQ ? 1 : 0,
            want_sums = flags & MIDAS_SITES_SUMS ? 1 : 0;
  const int S = n_samples;
  if ((per_gene && (!site_gene || n_genes_in < 0)) || (want_seq && (!out_seq || !minor || !major || seq_cap < 0)) ||
      (want_sums && (!out_pi || !out_snps || !out_sites || !out_depth)) || iparams8[4] < 0 || iparams8[5] < 0)
    return MIDAS_SNPS_ERR_INVALID_ARG;
  int n_cols = 0;
  for (int s = 0; s < S; ++s) {
    if (sample_col[s] < 0) return MIDAS_SNPS_ERR_INVALID_ARG;
    n_cols = std::max(n_cols, sample_col[s] + 1);
  }
  if (per_gene)
    for (int64_t i = 0; i < n_sites_max; ++i)
      if (site_gene[i] >= n_genes_in) return MIDAS_SNPS_ERR_INVALID_ARG;
  ctx->clear_error();
  ctx->err_read = -1;
  for (int k = 0; k < 16; ++k) out_stats16[k] = 0;
  out_stats16[4] = 0;
  out_stats16[5] = -1;
  out_stats16[6] = -1;
  if (out_ms8) for (int k = 0; k < 8; ++k) out_ms8[k] = 0.f;
  const long long n_genes = per_gene ? n_genes_in : 1;
  const long long chains = pooled ? 1 : S;
  const size_t n_acc = (size_t)(chains * n_genes);
  if (want_sums)
    for (size_t k = 0; k < n_acc; ++k) { out_pi[k] = 0.0; out_snps[k] = 0; out_sites[k] = 0; out_depth[k] = 0; }
  if (n_sites_max == 0) return MIDAS_SNPS_OK;
  std::vector<int32_t> col_slot((size_t)n_cols, -1);
  for (int s = 0; s < S; ++s) {
    if (col_slot[(size_t)sample_col[s]] >= 0) return ss_fail(ctx, MIDAS_SNPS_ERR_INVALID_ARG, "a matrix column is selected twice");
    col_slot[(size_t)sample_col[s]] = s;
  }
  SS_TRY(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const long long per_row = (long long)S * (8 + 8 + 1 + 2 * (long long)sizeof(SideCell) + (want_seq ? 1 : 0)) + 4 + 4 + 4 + 8 + 1 + 8 + 8;
  SsBufs dev;
  SsEvents ev;
  float ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};     // upload, index, parse, site, order, sums, seq, download
  RowGroups rg(ctx, dev, ev, ms, out_stats16);
  {
    // (max_sites 0: the reference converts the first row's cells and stops)
    const int32_t rc = rg.init(freq, freq_bytes, depth, depth_bytes, max_sites == 0 ? std::min<int64_t>(n_sites_max, 1) : n_sites_max, S,
                               col_slot, iparams8[4], iparams8[5], per_row);
    if (rc != MIDAS_SNPS_OK) return rc;
  }
  const long long G = rg.G;
  const size_t cells = rg.cells;
  double *d_fv = rg.d_fv, *d_pooled = nullptr, *d_mean = nullptr, *d_pi = nullptr;
  long long *d_dv = rg.d_dv, *d_last = nullptr, *d_snps = nullptr, *d_sites = nullptr, *d_depth = nullptr;
  uint8_t *d_cell = nullptr, *d_mask = nullptr, *d_final = nullptr, *d_seq = nullptr;
  uint32_t *d_keep = nullptr, *d_rank = nullptr, *d_scratch = rg.d_scratch;
  int32_t* d_gene = nullptr;
  char *d_minor = nullptr, *d_major = nullptr;
  unsigned long long *d_no_gene = nullptr, *d_err = nullptr;
  SS_TRY(dev.get(&d_err, 8));
  SS_TRY(dev.get(&d_cell, cells));
  SS_TRY(dev.get(&d_mask, (size_t)G));
  SS_TRY(dev.get(&d_final, (size_t)G));
  SS_TRY(dev.get(&d_keep, (size_t)G * 4));
  SS_TRY(dev.get(&d_rank, (size_t)G * 4));
  SS_TRY(dev.get(&d_pooled, (size_t)G * 8));
  SS_TRY(dev.get(&d_mean, (size_t)S * 8));
  SS_TRY(dev.get(&d_last, 8));
  SS_TRY(dev.get(&d_no_gene, 8));
  SS_TRY(hipMemsetAsync(d_no_gene, 0, 8, st));
  if (per_gene) SS_TRY(dev.get(&d_gene, (size_t)G * 4));
  if (want_seq) {
    SS_TRY(dev.get(&d_seq, cells));
    SS_TRY(dev.get(&d_minor, (size_t)G));
    SS_TRY(dev.get(&d_major, (size_t)G));
  }
  if (want_sums) {
    SS_TRY(dev.get(&d_pi, n_acc * 8));
    SS_TRY(dev.get(&d_snps, n_acc * 8));
    SS_TRY(dev.get(&d_sites, n_acc * 8));
    SS_TRY(dev.get(&d_depth, n_acc * 8));
    SS_TRY(hipMemsetAsync(d_pi, 0, n_acc * 8, st));
    SS_TRY(hipMemsetAsync(d_snps, 0, n_acc * 8, st));
    SS_TRY(hipMemsetAsync(d_sites, 0, n_acc * 8, st));
    SS_TRY(hipMemsetAsync(d_depth, 0, n_acc * 8, st));
  }
  SS_TRY(hipMemcpyAsync(d_mean, mean_depth, (size_t)S * 8, hipMemcpyHostToDevice, st));
  long long kept = 0;
  bool stop = false;
  while (!stop) {
    long long g = 0;
    {
      const int32_t rc = rg.next(&g);
      if (rc != MIDAS_SNPS_OK) return rc;
    }
    if (g == 0) break;
    const long long base = rg.base;
    // ---- site kernel, order, sums, sequences ---------------------------------------------------------------------------
    SS_TRY(hipMemcpyAsync(d_mask, site_mask + base, (size_t)g, hipMemcpyHostToDevice, st));
    if (per_gene) SS_TRY(hipMemcpyAsync(d_gene, site_gene + base, (size_t)g * 4, hipMemcpyHostToDevice, st));
    if (want_seq) {
      SS_TRY(hipMemcpyAsync(d_minor, minor + base, (size_t)g, hipMemcpyHostToDevice, st));
      SS_TRY(hipMemcpyAsync(d_major, major + base, (size_t)g, hipMemcpyHostToDevice, st));
    }
    SS_TRY(hipEventRecord(ev.e[3], st));
    SiteP sp;
    sp.fv = d_fv; sp.dv = d_dv; sp.cell = d_cell; sp.mean_depth = d_mean; sp.mask = d_mask; sp.g = g; sp.stride = G; sp.S = S;
    sp.site_depth = site_depth; sp.site_ratio = fparams5[0]; sp.allele_support = fparams5[1]; sp.site_prev = fparams5[2];
    sp.site_maf = fparams5[3]; sp.weight = weight; sp.round_freq = round_freq; sp.mask_only = mask_only; sp.keep = d_keep;
    sp.pooled = d_pooled; sp.err = d_err;
    SS_TRY(hipMemsetAsync(d_err, 0xFF, 8, st));
    hipLaunchKernelGGL(ss_site_kernel, dim3(nblocks(g, 256)), dim3(256), 0, st, sp);
    SS_TRY(hipGetLastError());
    SS_TRY(hipEventRecord(ev.e[4], st));
    uint32_t last_keep = 0, last_rank = 0;
    long long last_row = -1;
    SS_TRY(hipMemsetAsync(d_last, 0xFF, 8, st));
    SS_TRY(launch_scan_u32(d_keep, d_rank, g, d_scratch, st));
    hipLaunchKernelGGL(ss_order_kernel, dim3(nblocks(g, 256)), dim3(256), 0, st, d_keep, d_rank, g, kept, max_sites, d_final, d_last);
    SS_TRY(hipGetLastError());
    SS_TRY(hipEventRecord(ev.e[5], st));
    SS_TRY(hipMemcpyAsync(&last_keep, d_keep + g - 1, 4, hipMemcpyDeviceToHost, st));
    SS_TRY(hipMemcpyAsync(&last_rank, d_rank + g - 1, 4, hipMemcpyDeviceToHost, st));
    SS_TRY(hipMemcpyAsync(&last_row, d_last, 8, hipMemcpyDeviceToHost, st));
    unsigned long long err = kNoBad;
    SS_TRY(hipMemcpyAsync(&err, d_err, 8, hipMemcpyDeviceToHost, st));
    if (want_sums) {
      SumP q;
      q.fv = pooled ? d_pooled : d_fv; q.dv = d_dv; q.cell = d_cell; q.final_keep = d_final; q.gene = d_gene; q.g = g; q.stride = G;
      q.pooled = pooled; q.per_gene = per_gene; q.round_freq = round_freq; q.n_genes = n_genes; q.snp_maf = fparams5[4];
      q.pi = d_pi; q.snps = d_snps; q.sites = d_sites; q.depth = d_depth; q.no_gene = d_no_gene;
      hipLaunchKernelGGL(ss_sums_kernel, dim3((unsigned)chains), dim3(64), 0, st, q);
      SS_TRY(hipGetLastError());
    }
    SS_TRY(hipEventRecord(ev.e[6], st));
    if (want_seq) {
      hipLaunchKernelGGL(ss_seq_kernel, dim3(nblocks(g, 256)), dim3(256), 0, st, d_fv, d_dv, d_cell, d_final, d_rank, d_minor, d_major, g, G,
                         S, d_seq);
      SS_TRY(hipGetLastError());
    }
    SS_TRY(hipEventRecord(ev.e[7], st));
    SS_TRY(hipStreamSynchronize(st));
    SS_TRY(rg.lap(3, 4, 3));
    SS_TRY(rg.lap(4, 5, 4));
    SS_TRY(rg.lap(5, 6, 5));
    SS_TRY(rg.lap(6, 7, 6));
    long long kept_g = (long long)last_rank + last_keep;
    if (max_sites >= 0) kept_g = std::min(kept_g, max_sites - kept);
    // the rows the reference reads: all of the group, or up to the one after the row that fills max_sites -- whose cells it
    // converts, but whose pooled frequency it never forms
    {
      const long long read_rows = last_row >= 0 ? last_row + 2 : g;
      const long long pool_rows = max_sites == 0 ? 0 : last_row >= 0 ? last_row + 1 : g;
      if (err != kNoBad && (long long)(err >> 32) < pool_rows && call_error_comes_first(rg, read_rows, err))
        return site_pool_error(ctx, err, base, out_stats16);
      const int32_t rc = rg.check_rows(read_rows);
      if (rc != MIDAS_SNPS_OK) return rc;
    }
    SS_TRY(hipEventRecord(ev.e[0], st));
    if (dump_freq || dump_depth)
      for (int s = 0; s < S; ++s) {
        if (dump_freq) SS_TRY(hipMemcpyAsync(dump_freq + (size_t)s * n_sites_max + base, d_fv + (size_t)s * G, (size_t)g * 8, hipMemcpyDeviceToHost, st));
        if (dump_depth) SS_TRY(hipMemcpyAsync(dump_depth + (size_t)s * n_sites_max + base, d_dv + (size_t)s * G, (size_t)g * 8, hipMemcpyDeviceToHost, st));
      }
    if (dump_keep) SS_TRY(hipMemcpyAsync(dump_keep + base, d_final, (size_t)g, hipMemcpyDeviceToHost, st));
    if (dump_pooled) SS_TRY(hipMemcpyAsync(dump_pooled + base, d_pooled, (size_t)g * 8, hipMemcpyDeviceToHost, st));
    if (want_seq && kept_g > 0) {
      if (kept + kept_g > seq_cap) return ss_fail(ctx, MIDAS_SNPS_ERR_INVALID_ARG, "the retained sites do not fit the sequence capacity");
      SS_TRY(hipMemcpy2DAsync(out_seq + kept, (size_t)seq_cap, d_seq, (size_t)G, (size_t)kept_g, (size_t)S, hipMemcpyDeviceToHost, st));
    }
    SS_TRY(hipEventRecord(ev.e[1], st));
    SS_TRY(hipStreamSynchronize(st));
    SS_TRY(rg.lap(0, 1, 7));
    kept += kept_g;
    rg.advance(g);
    if (last_row >= 0) {
      stop = true;
      const int32_t rc = last_row == g - 1 ? rg.check_row_behind() : MIDAS_SNPS_OK;
      if (rc != MIDAS_SNPS_OK) return rc;
    }
  }
  if (want_sums) {
    SS_TRY(hipMemcpyAsync(out_pi, d_pi, n_acc * 8, hipMemcpyDeviceToHost, st));
    SS_TRY(hipMemcpyAsync(out_snps, d_snps, n_acc * 8, hipMemcpyDeviceToHost, st));
    SS_TRY(hipMemcpyAsync(out_sites, d_sites, n_acc * 8, hipMemcpyDeviceToHost, st));
    SS_TRY(hipMemcpyAsync(out_depth, d_depth, n_acc * 8, hipMemcpyDeviceToHost, st));
  }
  unsigned long long no_gene = 0;
  SS_TRY(hipMemcpyAsync(&no_gene, d_no_gene, 8, hipMemcpyDeviceToHost, st));
  SS_TRY(hipStreamSynchronize(st));
  out_stats16[0] = rg.base;
  out_stats16[1] = kept;
  out_stats16[7] = rg.groups;
  out_stats16[8] = (int64_t)no_gene;
  out_stats16[9] = G;
  out_stats16[10] = rg.chunk_bytes;
  if (out_ms8) for (int k = 0; k < 8; ++k) out_ms8[k] = ms[k];
  return MIDAS_SNPS_OK;
}

namespace {

// what the two strain_tracking.py entry points check and set up alike
int32_t strains_begin(midas_snps_ctx* ctx, const char* freq, int64_t freq_bytes, const char* depth, int64_t depth_bytes, int64_t n_parse,
                      int64_t n_call, int32_t n_samples, const int32_t* sample_col, const double* fparams2, const int64_t* iparams8,
                      int64_t* out_stats16, float* out_ms8, std::vector<int32_t>* col_slot) {
  if (!ctx || freq_bytes < 0 || depth_bytes < 0 || (freq_bytes > 0 && !freq) || (depth_bytes > 0 && !depth) || n_parse < 0 || n_call < 0 ||
      n_call > n_parse || n_parse > 0x7FFFFFFFll || n_samples < 1 || !sample_col || !fparams2 || !iparams8 || !out_stats16 || iparams8[2] < 0 ||
      iparams8[3] < 0 || iparams8[5] < 0)
    return MIDAS_SNPS_ERR_INVALID_ARG;
  int n_cols = 0;
  for (int s = 0; s < n_samples; ++s) {
    if (sample_col[s] < 0) return MIDAS_SNPS_ERR_INVALID_ARG;
    n_cols = std::max(n_cols, sample_col[s] + 1);
  }
  ctx->clear_error();
  ctx->err_read = -1;
  for (int k = 0; k < 16; ++k) out_stats16[k] = 0;
  out_stats16[5] = -1;
  out_stats16[6] = -1;
  if (out_ms8) for (int k = 0; k < 8; ++k) out_ms8[k] = 0.f;
  col_slot->assign((size_t)n_cols, -1);
  for (int s = 0; s < n_samples; ++s) {
    if ((*col_slot)[(size_t)sample_col[s]] >= 0) return ss_fail(ctx, MIDAS_SNPS_ERR_INVALID_ARG, "a matrix column is selected twice");
    (*col_slot)[(size_t)sample_col[s]] = s;
  }
  return MIDAS_SNPS_OK;
}

// a site that cannot be called (the reference raises there): its place in stats, the reason in words
int32_t strains_call_error(midas_snps_ctx* ctx, unsigned long long err, long long base, int64_t* stats) {
  const long long row = base + (long long)(err >> 32), slot = (long long)((err & 0xFFFFFFFFull) >> 2);
  const int why = (int)(err & 3u);
  stats[4] = 2 + why;
  stats[5] = row;
  stats[6] = slot;
  stats[0] = base;
  char buf[160];
  if (why == (int)kCallNonFinite) snprintf(buf, sizeof buf, "data row %lld, sample %lld: frequency x depth is not a finite number", row, slot);
  else snprintf(buf, sizeof buf, "data row %lld, sample %lld: the %s allele is none of A, T, C, G", row, slot, why == (int)kCallMinorLetter ? "minor" : "major");
  return ss_fail(ctx, MIDAS_SNPS_ERR_BAD_LAYOUT, buf);
}

}  // namespace

extern "C" int32_t midas_sites_id_markers(midas_snps_ctx* ctx, const char* freq, int64_t freq_bytes, const char* depth, int64_t depth_bytes,
                                          int64_t n_parse, int64_t n_call, const uint8_t* minor_code, const uint8_t* major_code,
                                          int32_t n_samples, const int32_t* sample_col, const double* fparams2, const int64_t* iparams8,
                                          int32_t* out_rows7, int64_t* out_stats16, float* out_ms8) {
  std::vector<int32_t> col_slot;
  {
    const int32_t rc = strains_begin(ctx, freq, freq_bytes, depth, depth_bytes, n_parse, n_call, n_samples, sample_col, fparams2, iparams8,
                                     out_stats16, out_ms8, &col_slot);
    if (rc != MIDAS_SNPS_OK) return rc;
  }
  if (n_call > 0 && (!minor_code || !major_code || !out_rows7)) return MIDAS_SNPS_ERR_INVALID_ARG;
  if (n_parse == 0) return MIDAS_SNPS_OK;
  const int S = n_samples;
  const long long capacity = iparams8[4];
  SS_TRY(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const long long per_row = (long long)S * (8 + 8 + 2 * (long long)sizeof(SideCell)) + 4 + 4 + 4 + 1 + 1 + 24 + 28;
  SsBufs dev;
  SsEvents ev;
  float ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};     // upload, index, parse, call, compact, -, -, download
  RowGroups rg(ctx, dev, ev, ms, out_stats16);
  {
    const int32_t rc = rg.init(freq, freq_bytes, depth, depth_bytes, n_parse, S, col_slot, iparams8[2], iparams8[3], per_row);
    if (rc != MIDAS_SNPS_OK) return rc;
  }
  const long long G = rg.G;
  uint8_t *d_minor = nullptr, *d_major = nullptr;
  uint32_t *d_flag = nullptr, *d_rank = nullptr;
  int32_t *d_row6 = nullptr, *d_out7 = nullptr;
  unsigned long long* d_err = nullptr;
  SS_TRY(dev.get(&d_minor, (size_t)G));
  SS_TRY(dev.get(&d_major, (size_t)G));
  SS_TRY(dev.get(&d_flag, (size_t)G * 4));
  SS_TRY(dev.get(&d_rank, (size_t)G * 4));
  SS_TRY(dev.get(&d_row6, (size_t)G * 24));
  SS_TRY(dev.get(&d_out7, (size_t)G * 28));
  SS_TRY(dev.get(&d_err, 8));
  long long found = 0;
  for (;;) {
    long long g = 0;
    {
      const int32_t rc = rg.next(&g);
      if (rc != MIDAS_SNPS_OK) return rc;
    }
    if (g == 0) break;
    const long long base = rg.base, gc = std::max<long long>(0, std::min<long long>(g, n_call - base));
    long long n = 0;
    unsigned long long err = kNoBad;
    if (gc > 0) {
      SS_TRY(hipMemcpyAsync(d_minor, minor_code + base, (size_t)gc, hipMemcpyHostToDevice, st));
      SS_TRY(hipMemcpyAsync(d_major, major_code + base, (size_t)gc, hipMemcpyHostToDevice, st));
      SS_TRY(hipMemsetAsync(d_err, 0xFF, 8, st));
      SS_TRY(hipEventRecord(ev.e[3], st));
      MarkP mp;
      mp.fv = rg.d_fv; mp.dv = rg.d_dv; mp.minor = d_minor; mp.major = d_major; mp.g = gc; mp.stride = G; mp.S = S;
      mp.min_freq = fparams2[0]; mp.min_reads = (double)iparams8[0]; mp.allele_prev = iparams8[1]; mp.flag = d_flag; mp.row6 = d_row6;
      mp.err = d_err;
      hipLaunchKernelGGL(ss_mark_kernel, dim3(nblocks(gc, 256)), dim3(256), 0, st, mp);
      SS_TRY(hipGetLastError());
      SS_TRY(hipEventRecord(ev.e[4], st));
      uint32_t last_flag = 0, last_rank = 0;
      SS_TRY(hipMemcpyAsync(&last_flag, d_flag + gc - 1, 4, hipMemcpyDeviceToHost, st));
      SS_TRY(launch_scan_u32(d_flag, d_rank, gc, rg.d_scratch, st));
      hipLaunchKernelGGL(ss_mark_compact_kernel, dim3(nblocks(gc, 256)), dim3(256), 0, st, d_flag, d_rank, d_row6, gc, base, d_out7);
      SS_TRY(hipGetLastError());
      SS_TRY(hipEventRecord(ev.e[5], st));
      SS_TRY(hipMemcpyAsync(&last_rank, d_rank + gc - 1, 4, hipMemcpyDeviceToHost, st));
      SS_TRY(hipMemcpyAsync(&err, d_err, 8, hipMemcpyDeviceToHost, st));
      SS_TRY(hipStreamSynchronize(st));
      SS_TRY(rg.lap(3, 4, 3));
      SS_TRY(rg.lap(4, 5, 4));
      n = (long long)last_rank + last_flag;
    }
    if (call_error_comes_first(rg, g, err)) return strains_call_error(ctx, err, base, out_stats16);
    {
      const int32_t rc = rg.check_rows(g);      // (n_parse ends with the last row the reference reads)
      if (rc != MIDAS_SNPS_OK) return rc;
    }
    if (n > 0) {
      if (found + n > capacity) return ss_fail(ctx, MIDAS_SNPS_ERR_INVALID_ARG, "the markers do not fit the output capacity");
      SS_TRY(hipEventRecord(ev.e[0], st));
      SS_TRY(hipMemcpyAsync(out_rows7 + 7 * found, d_out7, (size_t)n * 28, hipMemcpyDeviceToHost, st));
      SS_TRY(hipEventRecord(ev.e[1], st));
      SS_TRY(hipStreamSynchronize(st));
      SS_TRY(rg.lap(0, 1, 7));
      found += n;
    }
    rg.advance(g);
  }
  out_stats16[0] = rg.base;
  out_stats16[1] = found;
  out_stats16[7] = rg.groups;
  out_stats16[9] = G;
  out_stats16[10] = rg.chunk_bytes;
  if (out_ms8) for (int k = 0; k < 8; ++k) out_ms8[k] = ms[k];
  return MIDAS_SNPS_OK;
}

extern "C" int32_t midas_sites_track_markers(midas_snps_ctx* ctx, const char* freq, int64_t freq_bytes, const char* depth, int64_t depth_bytes,
                                             int64_t n_parse, int64_t n_call, const uint8_t* site_which, int32_t n_samples,
                                             const int32_t* sample_col, const double* fparams2, const int64_t* iparams8, int64_t* out_both,
                                             int64_t* out_stats16, float* out_ms8) {
  std::vector<int32_t> col_slot;
  {
    const int32_t rc = strains_begin(ctx, freq, freq_bytes, depth, depth_bytes, n_parse, n_call, n_samples, sample_col, fparams2, iparams8,
                                     out_stats16, out_ms8, &col_slot);
    if (rc != MIDAS_SNPS_OK) return rc;
  }
  if (!out_both || (n_call > 0 && !site_which)) return MIDAS_SNPS_ERR_INVALID_ARG;
  for (int64_t i = 0; i < n_call; ++i)
    if (site_which[i] > 2) return MIDAS_SNPS_ERR_INVALID_ARG;
  const int S = n_samples;
  const size_t n_acc = (size_t)S * (size_t)S;
  for (size_t k = 0; k < n_acc; ++k) out_both[k] = 0;
  if (n_parse == 0) return MIDAS_SNPS_OK;
  SS_TRY(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const long long per_row = (long long)S * (8 + 8 + 2 * (long long)sizeof(SideCell)) + 4 + 4 + 4 + 4 + 1 + (S + 7) / 8;
  SsBufs dev;
  SsEvents ev;
  float ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};     // upload, index, parse, matched sites, bit matrix, pairs, -, download
  RowGroups rg(ctx, dev, ev, ms, out_stats16);
  {
    const int32_t rc = rg.init(freq, freq_bytes, depth, depth_bytes, n_parse, S, col_slot, iparams8[2], iparams8[3], per_row);
    if (rc != MIDAS_SNPS_OK) return rc;
  }
  const long long G = rg.G, wstride = (G + 63) / 64;
  uint8_t* d_which = nullptr;
  uint32_t *d_flag = nullptr, *d_rank = nullptr, *d_list = nullptr;
  unsigned long long *d_bits = nullptr, *d_both = nullptr, *d_err = nullptr;
  SS_TRY(dev.get(&d_which, (size_t)G));
  SS_TRY(dev.get(&d_flag, (size_t)G * 4));
  SS_TRY(dev.get(&d_rank, (size_t)G * 4));
  SS_TRY(dev.get(&d_list, (size_t)G * 4));
  SS_TRY(dev.get(&d_bits, (size_t)S * (size_t)wstride * 8));
  SS_TRY(dev.get(&d_both, n_acc * 8));
  SS_TRY(dev.get(&d_err, 8));
  SS_TRY(hipMemsetAsync(d_both, 0, n_acc * 8, st));
  const int tiles_side = (S + kPairTile - 1) / kPairTile;
  const long long n_tiles = (long long)tiles_side * (tiles_side + 1) / 2;
  const long long pair_blocks = iparams8[5] > 0 ? iparams8[5] : 1024;      // workgroups the pair kernel aims at
  long long matched = 0, word_pairs = 0, max_runs = 0, max_steps = 0;
  for (;;) {
    long long g = 0;
    {
      const int32_t rc = rg.next(&g);
      if (rc != MIDAS_SNPS_OK) return rc;
    }
    if (g == 0) break;
    const long long base = rg.base, gc = std::max<long long>(0, std::min<long long>(g, n_call - base));
    unsigned long long err = kNoBad;
    if (gc > 0) {
      SS_TRY(hipMemcpyAsync(d_which, site_which + base, (size_t)gc, hipMemcpyHostToDevice, st));
      SS_TRY(hipEventRecord(ev.e[3], st));
      hipLaunchKernelGGL(ss_which_flag_kernel, dim3(nblocks(gc, 256)), dim3(256), 0, st, d_which, gc, d_flag);
      SS_TRY(hipGetLastError());
      uint32_t last_flag = 0, last_rank = 0;
      SS_TRY(hipMemcpyAsync(&last_flag, d_flag + gc - 1, 4, hipMemcpyDeviceToHost, st));
      SS_TRY(launch_scan_u32(d_flag, d_rank, gc, rg.d_scratch, st));
      hipLaunchKernelGGL(ss_which_list_kernel, dim3(nblocks(gc, 256)), dim3(256), 0, st, d_which, d_rank, gc, d_list);
      SS_TRY(hipGetLastError());
      SS_TRY(hipMemcpyAsync(&last_rank, d_rank + gc - 1, 4, hipMemcpyDeviceToHost, st));
      SS_TRY(hipEventRecord(ev.e[4], st));
      SS_TRY(hipStreamSynchronize(st));
      SS_TRY(rg.lap(3, 4, 3));
      const long long m = (long long)last_rank + last_flag, n_words = (m + 63) / 64;
      if (m > 0) {
        SS_TRY(hipMemsetAsync(d_err, 0xFF, 8, st));
        SS_TRY(hipEventRecord(ev.e[4], st));
        hipLaunchKernelGGL(ss_bits_kernel, dim3((unsigned)n_words, (unsigned)((S + 3) / 4)), dim3(256), 0, st, rg.d_fv, rg.d_dv, d_list, m, G, S,
                           fparams2[0], (double)iparams8[0], d_bits, wstride, d_err);
        SS_TRY(hipGetLastError());
        SS_TRY(hipEventRecord(ev.e[5], st));
        // word runs: enough workgroups to fill the device when the tiles are few, each run whole staging steps
        long long runs = std::max<long long>(1, std::min<long long>((pair_blocks + n_tiles - 1) / n_tiles, (n_words + kPairRun - 1) / kPairRun));
        runs = std::min<long long>(runs, 65535);
        const long long run_words = ((n_words + runs - 1) / runs + kPairRun - 1) / kPairRun * kPairRun;
        runs = (n_words + run_words - 1) / run_words;
        hipLaunchKernelGGL(ss_pairs_kernel, dim3((unsigned)n_tiles, (unsigned)runs), dim3(256), 0, st, d_bits, wstride, n_words, run_words, S,
                           tiles_side, d_both);
        SS_TRY(hipGetLastError());
        SS_TRY(hipEventRecord(ev.e[6], st));
        SS_TRY(hipMemcpyAsync(&err, d_err, 8, hipMemcpyDeviceToHost, st));
        SS_TRY(hipStreamSynchronize(st));
        SS_TRY(rg.lap(4, 5, 4));
        SS_TRY(rg.lap(5, 6, 5));
        matched += m;
        word_pairs += (long long)S * (S + 1) / 2 * n_words;
        max_runs = std::max(max_runs, runs);
        max_steps = std::max(max_steps, run_words / kPairRun);
      }
    }
    if (call_error_comes_first(rg, g, err)) return strains_call_error(ctx, err, base, out_stats16);
    {
      const int32_t rc = rg.check_rows(g);
      if (rc != MIDAS_SNPS_OK) return rc;
    }
    rg.advance(g);
  }
  SS_TRY(hipEventRecord(ev.e[0], st));
  SS_TRY(hipMemcpyAsync(out_both, d_both, n_acc * 8, hipMemcpyDeviceToHost, st));
  SS_TRY(hipEventRecord(ev.e[1], st));
  SS_TRY(hipStreamSynchronize(st));
  SS_TRY(rg.lap(0, 1, 7));
  out_stats16[0] = rg.base;
  out_stats16[1] = matched;
  out_stats16[7] = rg.groups;
  out_stats16[8] = word_pairs;
  out_stats16[11] = max_runs;
  out_stats16[12] = max_steps;
  out_stats16[9] = G;
  out_stats16[10] = rg.chunk_bytes;
  if (out_ms8) for (int k = 0; k < 8; ++k) out_ms8[k] = ms[k];
  return MIDAS_SNPS_OK;
}

// snp_trees.py: midas_sites_scan's site decisions under MIDAS_SITES_SEQ, then the planes and the pair counts of every group
extern "C" int32_t midas_sites_consensus_pairs(midas_snps_ctx* ctx, const char* freq, int64_t freq_bytes, const char* depth, int64_t depth_bytes,
                                               int64_t n_sites_max, const uint8_t* site_mask, int32_t n_samples, const int32_t* sample_col,
                                               const double* mean_depth, const double* fparams5, const int64_t* iparams8, int64_t* out_both,
                                               int64_t* out_diff, int64_t* out_stats16, float* out_ms8) {
  if (!ctx || freq_bytes < 0 || depth_bytes < 0 || (freq_bytes > 0 && !freq) || (depth_bytes > 0 && !depth) || n_sites_max < 0 ||
      n_samples < 1 || !sample_col || !mean_depth || !fparams5 || !iparams8 || !out_both || !out_diff || !out_stats16 ||
      (n_sites_max > 0 && !site_mask) || iparams8[4] < 0 || iparams8[5] < 0 || iparams8[6] < 0)
    return MIDAS_SNPS_ERR_INVALID_ARG;
  const long long site_depth = iparams8[0], max_sites = iparams8[1];
  const int mask_only = iparams8[2] & MIDAS_SITES_MASK_ONLY ? 1 : 0;
  const int S = n_samples;
  int n_cols = 0;
  for (int s = 0; s < S; ++s) {
    if (sample_col[s] < 0) return MIDAS_SNPS_ERR_INVALID_ARG;
    n_cols = std::max(n_cols, sample_col[s] + 1);
  }
  ctx->clear_error();
  ctx->err_read = -1;
  for (int k = 0; k < 16; ++k) out_stats16[k] = 0;
  out_stats16[5] = -1;
  out_stats16[6] = -1;
  if (out_ms8) for (int k = 0; k < 8; ++k) out_ms8[k] = 0.f;
  const size_t n_acc = (size_t)S * (size_t)S;
  for (size_t k = 0; k < n_acc; ++k) out_both[k] = out_diff[k] = 0;
  std::vector<int32_t> col_slot((size_t)n_cols, -1);
  for (int s = 0; s < S; ++s) {
    if (col_slot[(size_t)sample_col[s]] >= 0) return ss_fail(ctx, MIDAS_SNPS_ERR_INVALID_ARG, "a matrix column is selected twice");
    col_slot[(size_t)sample_col[s]] = s;
  }
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
  const long long G = rg.G, wstride = (G + 63) / 64;
  const size_t cells = rg.cells;
  double *d_pooled = nullptr, *d_mean = nullptr;
  long long* d_last = nullptr;
  uint8_t *d_cell = nullptr, *d_mask = nullptr, *d_final = nullptr;
  uint32_t *d_keep = nullptr, *d_rank = nullptr, *d_list = nullptr;
  unsigned long long *d_called = nullptr, *d_minor = nullptr, *d_both = nullptr, *d_diff = nullptr;
  SS_TRY(dev.get(&d_cell, cells));
  SS_TRY(dev.get(&d_mask, (size_t)G));
  SS_TRY(dev.get(&d_final, (size_t)G));
  SS_TRY(dev.get(&d_keep, (size_t)G * 4));
  SS_TRY(dev.get(&d_rank, (size_t)G * 4));
  SS_TRY(dev.get(&d_list, (size_t)G * 4));
  SS_TRY(dev.get(&d_pooled, (size_t)G * 8));
  SS_TRY(dev.get(&d_mean, (size_t)S * 8));
  SS_TRY(dev.get(&d_last, 8));
  SS_TRY(dev.get(&d_called, (size_t)S * (size_t)wstride * 8));
  SS_TRY(dev.get(&d_minor, (size_t)S * (size_t)wstride * 8));
  SS_TRY(dev.get(&d_both, n_acc * 8));
  SS_TRY(dev.get(&d_diff, n_acc * 8));
  SS_TRY(hipMemsetAsync(d_both, 0, n_acc * 8, st));
  SS_TRY(hipMemsetAsync(d_diff, 0, n_acc * 8, st));
  SS_TRY(hipMemcpyAsync(d_mean, mean_depth, (size_t)S * 8, hipMemcpyHostToDevice, st));
  const int tiles_side = (S + kPairTile - 1) / kPairTile;
  const long long n_tiles = (long long)tiles_side * (tiles_side + 1) / 2;
  const long long pair_blocks = iparams8[6] > 0 ? iparams8[6] : 1024;      // workgroups the pair kernel aims at
  long long kept = 0, word_pairs = 0, max_runs = 0, max_steps = 0;
  bool stop = false;
  while (!stop) {
    long long g = 0;
    {
      const int32_t rc = rg.next(&g);
      if (rc != MIDAS_SNPS_OK) return rc;
    }
    if (g == 0) break;
    const long long base = rg.base;
    SS_TRY(hipMemcpyAsync(d_mask, site_mask + base, (size_t)g, hipMemcpyHostToDevice, st));
    SS_TRY(hipEventRecord(ev.e[3], st));
    SiteP sp;
    sp.fv = rg.d_fv; sp.dv = rg.d_dv; sp.cell = d_cell; sp.mean_depth = d_mean; sp.mask = d_mask; sp.g = g; sp.stride = G; sp.S = S;
    sp.site_depth = site_depth; sp.site_ratio = fparams5[0]; sp.allele_support = fparams5[1]; sp.site_prev = fparams5[2];
    sp.site_maf = fparams5[3]; sp.weight = 0; sp.round_freq = 0; sp.mask_only = mask_only; sp.keep = d_keep; sp.pooled = d_pooled;
    sp.err = nullptr;                            // (neither rounded nor weighted: nothing the reference raises on)
    hipLaunchKernelGGL(ss_site_kernel, dim3(nblocks(g, 256)), dim3(256), 0, st, sp);
    SS_TRY(hipGetLastError());
    SS_TRY(hipEventRecord(ev.e[4], st));
    uint32_t last_keep = 0, last_rank = 0;
    long long last_row = -1;
    SS_TRY(hipMemsetAsync(d_last, 0xFF, 8, st));
    SS_TRY(launch_scan_u32(d_keep, d_rank, g, rg.d_scratch, st));
    hipLaunchKernelGGL(ss_order_kernel, dim3(nblocks(g, 256)), dim3(256), 0, st, d_keep, d_rank, g, kept, max_sites, d_final, d_last);
    SS_TRY(hipGetLastError());
    hipLaunchKernelGGL(ss_keep_list_kernel, dim3(nblocks(g, 256)), dim3(256), 0, st, d_final, d_rank, g, d_list);
    SS_TRY(hipGetLastError());
    SS_TRY(hipMemcpyAsync(&last_keep, d_keep + g - 1, 4, hipMemcpyDeviceToHost, st));
    SS_TRY(hipMemcpyAsync(&last_rank, d_rank + g - 1, 4, hipMemcpyDeviceToHost, st));
    SS_TRY(hipMemcpyAsync(&last_row, d_last, 8, hipMemcpyDeviceToHost, st));
    SS_TRY(hipStreamSynchronize(st));
    long long kept_g = (long long)last_rank + last_keep;
    if (max_sites >= 0) kept_g = std::min(kept_g, max_sites - kept);
    const long long n_words = (kept_g + 63) / 64;
    if (kept_g > 0) {
      hipLaunchKernelGGL(ss_planes_kernel, dim3((unsigned)n_words, (unsigned)((S + 3) / 4)), dim3(256), 0, st, rg.d_fv, rg.d_dv, d_cell, d_list,
                         kept_g, G, S, d_called, d_minor, wstride);
      SS_TRY(hipGetLastError());
    }
    SS_TRY(hipEventRecord(ev.e[5], st));
    if (kept_g > 0) {
      // word runs: enough workgroups to fill the device when the tiles are few, each run whole staging steps
      long long runs = std::max<long long>(1, std::min<long long>((pair_blocks + n_tiles - 1) / n_tiles, (n_words + kPlaneRun - 1) / kPlaneRun));
      runs = std::min<long long>(runs, 65535);
      const long long run_words = ((n_words + runs - 1) / runs + kPlaneRun - 1) / kPlaneRun * kPlaneRun;
      runs = (n_words + run_words - 1) / run_words;
      hipLaunchKernelGGL(ss_plane_pairs_kernel, dim3((unsigned)n_tiles, (unsigned)runs), dim3(256), 0, st, d_called, d_minor, wstride, n_words,
                         run_words, S, tiles_side, d_both, d_diff);
      SS_TRY(hipGetLastError());
      word_pairs += (long long)S * (S + 1) / 2 * n_words;
      max_runs = std::max(max_runs, runs);
      max_steps = std::max(max_steps, run_words / kPlaneRun);
    }
    SS_TRY(hipEventRecord(ev.e[6], st));
    SS_TRY(hipStreamSynchronize(st));
    SS_TRY(rg.lap(3, 4, 3));
    SS_TRY(rg.lap(4, 5, 4));
    SS_TRY(rg.lap(5, 6, 5));
    // the rows the reference reads: all of the group, or up to the one after the row that fills max_sites
    {
      const int32_t rc = rg.check_rows(last_row >= 0 ? last_row + 2 : g);
      if (rc != MIDAS_SNPS_OK) return rc;
    }
    kept += kept_g;
    rg.advance(g);
    if (last_row >= 0) {
      stop = true;
      const int32_t rc = last_row == g - 1 ? rg.check_row_behind() : MIDAS_SNPS_OK;
      if (rc != MIDAS_SNPS_OK) return rc;
    }
  }
  SS_TRY(hipEventRecord(ev.e[0], st));
  SS_TRY(hipMemcpyAsync(out_both, d_both, n_acc * 8, hipMemcpyDeviceToHost, st));
  SS_TRY(hipMemcpyAsync(out_diff, d_diff, n_acc * 8, hipMemcpyDeviceToHost, st));
  SS_TRY(hipEventRecord(ev.e[1], st));
  SS_TRY(hipStreamSynchronize(st));
  SS_TRY(rg.lap(0, 1, 7));
  out_stats16[0] = rg.base;
  out_stats16[1] = kept;
  out_stats16[7] = rg.groups;
  out_stats16[8] = word_pairs;
  out_stats16[9] = G;
  out_stats16[10] = rg.chunk_bytes;
  out_stats16[11] = max_runs;
  out_stats16[12] = max_steps;
  if (out_ms8) for (int k = 0; k < 8; ++k) out_ms8[k] = ms[k];
  return MIDAS_SNPS_OK;
}
