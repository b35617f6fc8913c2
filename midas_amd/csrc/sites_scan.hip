// snp_diversity.py / call_consensus.py on MI355X: the per-site loop of midas/analyze/parse_snps.py and of the
// two scripts over it, for all rows of snps_freq.txt / snps_depth.txt at once.
//
//   chunks, index, parse   the rows of the two matrices, a group at a time (RowGroups, sites_rows.h)
//   site, order            the site's decisions and --max_sites (SiteStep, sites_call.h)
//   resample --rand_reads: the reads of every retained variable site drawn again, its pooled frequency formed again
//            (sites_resample.h; midas_sites_scan_resampled only)
//   sums     one wave a chain (a sample, or the pool): 64 rows loaded coalesced, then folded in lane order -- the fp64 sum
//            is the sequential one, bit for bit; per-gene chains switch accumulators where the gene index changes.
//            Accumulators live in device memory and carry from group to group
//   classes  midas_sites_scan_classes: the sums once per site class in one pass, one wave a (chain, class); only pi is folded
//            in lane order, the integer sums come from ballots and per-lane partial sums (ss_sums_classes_kernel)
//   seq      call_consensus.py: one byte per (retained site, sample), sample-major
// strain_tracking.py walks the same rows in sites_strains.hip, snp_trees.py the same rows and site decisions in sites_trees.hip.
// This file is compiled with -ffp-contract=off (build.py): 2*f*(1-f) and d*f round as the interpreter rounds them.
#include "sites_call.h"
#include "sites_resample.h"

namespace midas {
namespace {

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

// ---- the sums per site class (midas_sites_scan_classes) ------------------------------------------------------------------------
struct ClassSumP {
  SumP s;                      // pi / snps / sites / depth are [classes][chains][n_genes]
  const uint8_t* site_class;   // [g], or nullptr: every row is class 0
};

// what one lane reads of one row, before anything is decided from it
struct ClassRow {
  double f;
  long long d;
  int gi;
  uint8_t keep, cls, cell;
};

// r < p.g.  Every load is unconditional, so that a step's loads can all be in flight while the step before it is folded
__device__ __forceinline__ ClassRow class_row_load(const ClassSumP& q, int chain, long long r) {
  const SumP& p = q.s;
  ClassRow w;
  const long long at = (long long)chain * p.stride + r;
  w.keep = p.final_keep[r];
  w.cls = q.site_class ? q.site_class[r] : (uint8_t)0;
  w.cell = p.pooled ? (uint8_t)1 : p.cell[at];
  w.f = p.pooled ? p.fv[r] : p.fv[at];
  w.d = p.pooled ? 0 : p.dv[at];
  w.gi = p.per_gene ? p.gene[r] : 0;
  return w;
}

__device__ __forceinline__ long long wave_sum_i64(long long v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// One wave per (chain, class): blockIdx.x the chain, blockIdx.y the class.  The chains of the classes share no accumulator, so
// they fold side by side.  Of a step's 64 rows the wave's live lanes are its class's alone, cut into runs of one gene (a run ends
// where the gene index changes; genome-wide a step is one run).  Per run:
//   pi      folded serially in lane order, two readlanes and one add a lane -- the sequential fp64 sum, bit for bit
//   sites, snps   popcounts of ballots
//   depth   a per-lane partial sum, reduced over the wave when the accumulators are written: where the gene changes and at the end
// Integer addition has no order, so these three need not ride the chain.  The next step's rows are loaded before the current
// step is folded.  Kept sites without a gene id are counted by chain 0 of class 0, whatever their class.
__global__ __launch_bounds__(64) void ss_sums_classes_kernel(ClassSumP q) {
  const SumP& p = q.s;
  if (p.g <= 0) return;
  const int chain = blockIdx.x, cls = blockIdx.y, lane = threadIdx.x;
  const long long base = ((long long)cls * gridDim.x + chain) * p.n_genes;
  const bool count_lost = p.per_gene && chain == 0 && cls == 0;
  long long cur = p.per_gene ? -1 : 0;
  double pi = 0.0;
  long long snps = 0, sites = 0, depth = 0, dpart = 0;
  unsigned long long lost = 0;
  if (!p.per_gene) { pi = p.pi[base]; snps = p.snps[base]; sites = p.sites[base]; depth = p.depth[base]; }
  const long long last = p.g - 1;
  ClassRow nx = class_row_load(q, chain, lane < last ? lane : last);
  for (long long r0 = 0; r0 < p.g; r0 += 64) {
    const ClassRow w = nx;
    if (r0 + 64 < p.g) {
      const long long rn = r0 + 64 + lane;
      nx = class_row_load(q, chain, rn < last ? rn : last);
    }
    const bool in = r0 + lane < p.g, kept = in && w.keep != 0;
    if (count_lost) lost += (unsigned long long)__popcll((long long)__ballot(kept && w.gi < 0));
    const bool on = kept && w.cls == cls && (w.cell & 1) != 0 && w.gi >= 0;
    double f = w.f;
    if (!p.pooled && p.round_freq) f = rint(f) + 0.0;
    const double term = (2.0 * f) * (1.0 - f);
    double m = f;                               // min(f, 1 - f) as Python's min
    if (1.0 - f < m) m = 1.0 - f;
    const long long d = on ? w.d : 0;
    unsigned long long live = __ballot(on);
    const unsigned long long snp_b = __ballot(on && m >= p.snp_maf);
    const int tlo = __double2loint(term), thi = __double2hiint(term);
    while (live) {
      // the run: the live lanes in front of the first live lane with another gene
      const int k0 = __ffsll((long long)live) - 1;
      const long long gk = __builtin_amdgcn_readlane(w.gi, k0);
      const unsigned long long other = live & ~__ballot(on && w.gi == (int)gk);
      unsigned long long run = other ? live & ((1ull << (__ffsll((long long)other) - 1)) - 1ull) : live;
      live &= ~run;
      if (gk != cur) {
        if (cur >= 0) {
          depth += wave_sum_i64(dpart);
          dpart = 0;
          if (lane == 0) { p.pi[base + cur] = pi; p.snps[base + cur] = snps; p.sites[base + cur] = sites; p.depth[base + cur] = depth; }
        }
        cur = gk;
        pi = p.pi[base + cur]; snps = p.snps[base + cur]; sites = p.sites[base + cur]; depth = p.depth[base + cur];
        // vmcnt(0) here, where the gene changes: loads return in order, so a wait for these four in the fold below would be a wait
        // for the next step's rows in every step, with or without a change
        __builtin_amdgcn_s_waitcnt(0x0F70);
      }
      sites += __popcll((long long)run);
      snps += __popcll((long long)(run & snp_b));
      if ((run >> lane) & 1ull) dpart += d;
      while (run) {
        const int k = __ffsll((long long)run) - 1;
        run &= run - 1;
        pi += __hiloint2double(__builtin_amdgcn_readlane(thi, k), __builtin_amdgcn_readlane(tlo, k));
      }
    }
  }
  if (cur >= 0) {
    depth += wave_sum_i64(dpart);
    if (lane == 0) { p.pi[base + cur] = pi; p.snps[base + cur] = snps; p.sites[base + cur] = sites; p.depth[base + cur] = depth; }
  }
  if (count_lost && lane == 0 && lost) atomicAdd(p.no_gene, lost);
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

// --rand_reads as midas_sites_scan_resampled takes it; midas_sites_scan passes none
struct ResampleArgs {
  int64_t rand_reads;
  int32_t replace;
  const uint32_t* mt_key;
  int32_t mt_pos;
  uint32_t* mt_key_out;
  int32_t* mt_pos_out;
  double* out_draw8;
};

// the entry points' common body.  site_class / n_classes: the class of every row and their number (nullptr, 1: one class);
// classed: the sums are midas_sites_scan_classes' -- [n_classes][chains][n_genes], by ss_sums_classes_kernel
int32_t sites_scan_body(midas_snps_ctx* ctx, const char* freq, int64_t freq_bytes, const char* depth, int64_t depth_bytes,
                        int64_t n_sites_max, const uint8_t* site_mask, const int32_t* site_gene, const char* minor,
                        const char* major, int32_t n_samples, const int32_t* sample_col, const double* mean_depth,
                        const double* fparams5, const int64_t* iparams8, double* out_pi, int64_t* out_snps,
                        int64_t* out_sites, int64_t* out_depth, uint8_t* out_seq, double* dump_freq, int64_t* dump_depth,
                        uint8_t* dump_keep, double* dump_pooled, int64_t* out_stats16, float* out_ms8, const ResampleArgs* ra,
                        const uint8_t* site_class, int32_t n_classes, bool classed) {
  if (!mean_depth || !fparams5 || !iparams8 || (n_sites_max > 0 && !site_mask)) return MIDAS_SNPS_ERR_INVALID_ARG;
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
  if (per_gene)
    for (int64_t i = 0; i < n_sites_max; ++i)
      if (site_gene[i] >= n_genes_in) return MIDAS_SNPS_ERR_INVALID_ARG;
  if (n_classes < 1 || n_classes > MIDAS_SITES_MAX_CLASSES || (n_classes > 1 && !site_class) || (classed && want_seq)) return MIDAS_SNPS_ERR_INVALID_ARG;
  if (site_class)
    for (int64_t i = 0; i < n_sites_max; ++i)
      if (site_mask[i] && site_class[i] >= n_classes) return MIDAS_SNPS_ERR_INVALID_ARG;
  std::vector<int32_t> col_slot;
  {
    const int32_t rc = sites_begin(ctx, freq, freq_bytes, depth, depth_bytes, n_sites_max, S, sample_col, out_stats16, out_ms8, &col_slot);
    if (rc != MIDAS_SNPS_OK) return rc;
  }
  const long long n_genes = per_gene ? n_genes_in : 1;
  const long long chains = pooled ? 1 : S;
  const size_t n_acc = (size_t)(chains * n_genes) * (size_t)n_classes;
  if (want_sums)
    for (size_t k = 0; k < n_acc; ++k) { out_pi[k] = 0.0; out_snps[k] = 0; out_sites[k] = 0; out_depth[k] = 0; }
  if (n_sites_max == 0) return MIDAS_SNPS_OK;
  SS_TRY(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const long long per_row = (long long)S * (8 + 8 + 1 + 2 * (long long)sizeof(SideCell) + (want_seq ? 1 : 0)) + 4 + 4 + 4 + 8 + 1 + 8 + 8 + (site_class ? 1 : 0) +
                            (ra ? ResampleStep::per_row(S) : 0);
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
  SiteStep site(ctx, rg, site_mask, site_depth, max_sites, fparams5, weight, round_freq, mask_only);
  {
    const int32_t rc = site.init(mean_depth, true);
    if (rc != MIDAS_SNPS_OK) return rc;
  }
  std::unique_ptr<ResampleStep> rs;
  if (ra) {
    rs.reset(new ResampleStep(ctx, rg, site, ra->rand_reads, ra->replace));
    const int32_t rc = rs->init(iparams8[7], ra->mt_key, ra->mt_pos);
    if (rc != MIDAS_SNPS_OK) return rc;
  }
  const long long G = rg.G;
  double *d_fv = rg.d_fv, *d_pi = nullptr;
  long long *d_dv = rg.d_dv, *d_snps = nullptr, *d_sites = nullptr, *d_depth = nullptr;
  uint8_t* d_seq = nullptr;
  int32_t* d_gene = nullptr;
  uint8_t* d_class = nullptr;
  char *d_minor = nullptr, *d_major = nullptr;
  unsigned long long* d_no_gene = nullptr;
  SS_TRY(dev.get(&d_no_gene, 8));
  SS_TRY(hipMemsetAsync(d_no_gene, 0, 8, st));
  if (per_gene) SS_TRY(dev.get(&d_gene, (size_t)G * 4));
  if (site_class) SS_TRY(dev.get(&d_class, (size_t)G));
  if (want_seq) {
    SS_TRY(dev.get(&d_seq, rg.cells));
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
    if (per_gene) SS_TRY(hipMemcpyAsync(d_gene, site_gene + base, (size_t)g * 4, hipMemcpyHostToDevice, st));
    if (site_class) SS_TRY(hipMemcpyAsync(d_class, site_class + base, (size_t)g, hipMemcpyHostToDevice, st));
    if (want_seq) {
      SS_TRY(hipMemcpyAsync(d_minor, minor + base, (size_t)g, hipMemcpyHostToDevice, st));
      SS_TRY(hipMemcpyAsync(d_major, major + base, (size_t)g, hipMemcpyHostToDevice, st));
    }
    {
      const int32_t rc = site.run(g);
      if (rc != MIDAS_SNPS_OK) return rc;
    }
    if (rs) {
      const int32_t rc = rs->run(g);
      if (rc != MIDAS_SNPS_OK) return rc;
    }
    if (want_sums) {
      SumP q;
      q.fv = pooled ? site.d_pooled : d_fv; q.dv = d_dv; q.cell = site.d_cell; q.final_keep = site.d_final; q.gene = d_gene; q.g = g;
      q.stride = G; q.pooled = pooled; q.per_gene = per_gene; q.round_freq = round_freq; q.n_genes = n_genes; q.snp_maf = fparams5[4];
      q.pi = d_pi; q.snps = d_snps; q.sites = d_sites; q.depth = d_depth; q.no_gene = d_no_gene;
      if (classed) {
        ClassSumP cq;
        cq.s = q; cq.site_class = d_class;
        hipLaunchKernelGGL(ss_sums_classes_kernel, dim3((unsigned)chains, (unsigned)n_classes), dim3(64), 0, st, cq);
      } else {
        hipLaunchKernelGGL(ss_sums_kernel, dim3((unsigned)chains), dim3(64), 0, st, q);
      }
      SS_TRY(hipGetLastError());
    }
    SS_TRY(hipEventRecord(ev.e[6], st));
    if (want_seq) {
      hipLaunchKernelGGL(ss_seq_kernel, dim3(nblocks(g, 256)), dim3(256), 0, st, d_fv, d_dv, site.d_cell, site.d_final, site.d_rank, d_minor,
                         d_major, g, G, S, d_seq);
      SS_TRY(hipGetLastError());
    }
    SS_TRY(hipEventRecord(ev.e[7], st));
    SS_TRY(hipStreamSynchronize(st));
    SS_TRY(rg.lap(3, 4, 3));
    SS_TRY(rg.lap(4, 5, 4));
    if (rs) {                                   // (the sums start behind the resampling pass, not behind the order)
      float t = 0.f;
      SS_TRY(hipEventElapsedTime(&t, rs->e[7], ev.e[6]));
      ms[5] += t;
      const int32_t rc = rs->collect();
      if (rc != MIDAS_SNPS_OK) return rc;
    } else {
      SS_TRY(rg.lap(5, 6, 5));
    }
    SS_TRY(rg.lap(6, 7, 6));
    {
      const int32_t rc = site.check_rows();
      if (rc != MIDAS_SNPS_OK) return rc;
    }
    const long long kept = site.kept, kept_g = site.kept_g();
    SS_TRY(hipEventRecord(ev.e[0], st));
    if (dump_freq || dump_depth)
      for (int s = 0; s < S; ++s) {
        if (dump_freq) SS_TRY(hipMemcpyAsync(dump_freq + (size_t)s * n_sites_max + base, d_fv + (size_t)s * G, (size_t)g * 8, hipMemcpyDeviceToHost, st));
        if (dump_depth) SS_TRY(hipMemcpyAsync(dump_depth + (size_t)s * n_sites_max + base, d_dv + (size_t)s * G, (size_t)g * 8, hipMemcpyDeviceToHost, st));
      }
    if (dump_keep) SS_TRY(hipMemcpyAsync(dump_keep + base, site.d_final, (size_t)g, hipMemcpyDeviceToHost, st));
    if (dump_pooled) SS_TRY(hipMemcpyAsync(dump_pooled + base, site.d_pooled, (size_t)g * 8, hipMemcpyDeviceToHost, st));
    if (want_seq && kept_g > 0) {
      if (kept + kept_g > seq_cap) return ss_fail(ctx, MIDAS_SNPS_ERR_INVALID_ARG, "the retained sites do not fit the sequence capacity");
      SS_TRY(hipMemcpy2DAsync(out_seq + kept, (size_t)seq_cap, d_seq, (size_t)G, (size_t)kept_g, (size_t)S, hipMemcpyDeviceToHost, st));
    }
    SS_TRY(hipEventRecord(ev.e[1], st));
    SS_TRY(hipStreamSynchronize(st));
    SS_TRY(rg.lap(0, 1, 7));
    {
      const int32_t rc = site.advance(&stop);
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
  out_stats16[1] = site.kept;
  out_stats16[8] = (int64_t)no_gene;
  if (rs) {
    const int32_t rc = rs->finish(ra->mt_key_out, ra->mt_pos_out, ra->out_draw8, out_stats16);
    if (rc != MIDAS_SNPS_OK) return rc;
  }
  sites_end(rg, out_ms8);
  return MIDAS_SNPS_OK;
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
  return sites_scan_body(ctx, freq, freq_bytes, depth, depth_bytes, n_sites_max, site_mask, site_gene, minor, major, n_samples, sample_col,
                         mean_depth, fparams5, iparams8, out_pi, out_snps, out_sites, out_depth, out_seq, dump_freq, dump_depth, dump_keep,
                         dump_pooled, out_stats16, out_ms8, nullptr, nullptr, 1, false);
}

extern "C" int32_t midas_sites_scan_resampled(midas_snps_ctx* ctx, const char* freq, int64_t freq_bytes, const char* depth, int64_t depth_bytes,
                                              int64_t n_sites_max, const uint8_t* site_mask, const int32_t* site_gene, const char* minor,
                                              const char* major, int32_t n_samples, const int32_t* sample_col, const double* mean_depth,
                                              const double* fparams5, const int64_t* iparams8, double* out_pi, int64_t* out_snps,
                                              int64_t* out_sites, int64_t* out_depth, uint8_t* out_seq, double* dump_freq, int64_t* dump_depth,
                                              uint8_t* dump_keep, double* dump_pooled, int64_t* out_stats16, float* out_ms8, int64_t rand_reads,
                                              int32_t replace, const uint32_t* mt_key, int32_t mt_pos, uint32_t* mt_key_out, int32_t* mt_pos_out,
                                              double* out_draw8) {
  if (rand_reads < 1 || rand_reads > kDrawMaxReads || !mt_key || mt_pos < 0 || mt_pos > 624 || !mt_key_out || !mt_pos_out || !iparams8 ||
      iparams8[7] < 0 || (iparams8[2] & MIDAS_SITES_SEQ))
    return MIDAS_SNPS_ERR_INVALID_ARG;
  // (an early return of the body -- no sites, an error -- leaves the stream where it was)
  for (int i = 0; i < 624; ++i) mt_key_out[i] = mt_key[i];
  *mt_pos_out = mt_pos;
  if (out_draw8) for (int i = 0; i < 8; ++i) out_draw8[i] = 0.0;
  const ResampleArgs ra{rand_reads, replace, mt_key, mt_pos, mt_key_out, mt_pos_out, out_draw8};
  return sites_scan_body(ctx, freq, freq_bytes, depth, depth_bytes, n_sites_max, site_mask, site_gene, minor, major, n_samples, sample_col,
                         mean_depth, fparams5, iparams8, out_pi, out_snps, out_sites, out_depth, out_seq, dump_freq, dump_depth, dump_keep,
                         dump_pooled, out_stats16, out_ms8, &ra, nullptr, 1, false);
}

extern "C" int32_t midas_sites_scan_classes(midas_snps_ctx* ctx, const char* freq, int64_t freq_bytes, const char* depth, int64_t depth_bytes,
                                            int64_t n_sites_max, const uint8_t* site_mask, const int32_t* site_gene, const char* minor,
                                            const char* major, int32_t n_samples, const int32_t* sample_col, const double* mean_depth,
                                            const double* fparams5, const int64_t* iparams8, double* out_pi, int64_t* out_snps,
                                            int64_t* out_sites, int64_t* out_depth, uint8_t* out_seq, double* dump_freq, int64_t* dump_depth,
                                            uint8_t* dump_keep, double* dump_pooled, int64_t* out_stats16, float* out_ms8,
                                            const uint8_t* site_class, int32_t n_classes) {
  return sites_scan_body(ctx, freq, freq_bytes, depth, depth_bytes, n_sites_max, site_mask, site_gene, minor, major, n_samples, sample_col,
                         mean_depth, fparams5, iparams8, out_pi, out_snps, out_sites, out_depth, out_seq, dump_freq, dump_depth, dump_keep,
                         dump_pooled, out_stats16, out_ms8, nullptr, site_class, n_classes, true);
}
