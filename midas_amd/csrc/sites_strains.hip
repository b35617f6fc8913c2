// strain_tracking.py (midas/analyze/track_strains.py) on MI355X: marker alleles and their sharing between samples.  It walks
// the rows of snps_freq.txt / snps_depth.txt as midas_sites_scan does (RowGroups, sites_rows.h: chunks, index, parse, side lists):
//   mark     id_markers: one thread a row counts the samples that have the minor, the major, both alleles and any read
//            (x >= min_freq and round(x * depth) >= min_reads), folds them onto A, T, C, G and decides the marker; the scan
//            compacts the marker rows
//   bits     track_markers: the matched sites of a group (one byte a site from the host: none, major, minor) are ranked by the
//            scan; one wave calls 64 of them for one sample, its ballot is a word of the bit matrix [sample][word]
//   pairs    both[i][j] += popcount(B[i][w] & B[j][w]) in 64 x 64 tiles of sample pairs staged through LDS; integer sums, held
//            on the device across groups (ss_pairs_kernel, text_rows.h)
// This file is compiled with -ffp-contract=off (build.py): x*depth rounds as the interpreter rounds it.
#include "sites_rows.h"

namespace midas {
namespace {

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

// what the two entry points check of their own before sites_begin
bool strains_args_ok(int64_t n_parse, int64_t n_call, const double* fparams2, const int64_t* iparams8) {
  return n_call >= 0 && n_call <= n_parse && n_parse <= 0x7FFFFFFFll && fparams2 && iparams8 && iparams8[2] >= 0 && iparams8[3] >= 0 &&
         iparams8[5] >= 0;
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
}  // namespace midas

using namespace midas;

extern "C" int32_t midas_sites_id_markers(midas_snps_ctx* ctx, const char* freq, int64_t freq_bytes, const char* depth, int64_t depth_bytes,
                                          int64_t n_parse, int64_t n_call, const uint8_t* minor_code, const uint8_t* major_code,
                                          int32_t n_samples, const int32_t* sample_col, const double* fparams2, const int64_t* iparams8,
                                          int32_t* out_rows7, int64_t* out_stats16, float* out_ms8) {
  if (!strains_args_ok(n_parse, n_call, fparams2, iparams8)) return MIDAS_SNPS_ERR_INVALID_ARG;
  std::vector<int32_t> col_slot;
  {
    const int32_t rc = sites_begin(ctx, freq, freq_bytes, depth, depth_bytes, n_parse, n_samples, sample_col, out_stats16, out_ms8, &col_slot);
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
  out_stats16[1] = found;
  sites_end(rg, out_ms8);
  return MIDAS_SNPS_OK;
}

extern "C" int32_t midas_sites_track_markers(midas_snps_ctx* ctx, const char* freq, int64_t freq_bytes, const char* depth, int64_t depth_bytes,
                                             int64_t n_parse, int64_t n_call, const uint8_t* site_which, int32_t n_samples,
                                             const int32_t* sample_col, const double* fparams2, const int64_t* iparams8, int64_t* out_both,
                                             int64_t* out_stats16, float* out_ms8) {
  if (!strains_args_ok(n_parse, n_call, fparams2, iparams8)) return MIDAS_SNPS_ERR_INVALID_ARG;
  std::vector<int32_t> col_slot;
  {
    const int32_t rc = sites_begin(ctx, freq, freq_bytes, depth, depth_bytes, n_parse, n_samples, sample_col, out_stats16, out_ms8, &col_slot);
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
  const PairTiles tiles = pair_tiles(S, kPairTile);
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
        const PairRuns pr = pair_runs(n_words, tiles.n, pair_blocks, kPairRun);
        hipLaunchKernelGGL(ss_pairs_kernel, dim3((unsigned)tiles.n, (unsigned)pr.runs), dim3(256), 0, st, d_bits, wstride, n_words, pr.run_words,
                           S, tiles.side, d_both);
        SS_TRY(hipGetLastError());
        SS_TRY(hipEventRecord(ev.e[6], st));
        SS_TRY(hipMemcpyAsync(&err, d_err, 8, hipMemcpyDeviceToHost, st));
        SS_TRY(hipStreamSynchronize(st));
        SS_TRY(rg.lap(4, 5, 4));
        SS_TRY(rg.lap(5, 6, 5));
        matched += m;
        word_pairs += (long long)S * (S + 1) / 2 * n_words;
        max_runs = std::max(max_runs, pr.runs);
        max_steps = std::max(max_steps, pr.run_words / kPairRun);
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
  out_stats16[1] = matched;
  out_stats16[8] = word_pairs;
  out_stats16[11] = max_runs;
  out_stats16[12] = max_steps;
  sites_end(rg, out_ms8);
  return MIDAS_SNPS_OK;
}
