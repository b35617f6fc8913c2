// run_species.py, the classify step (midas/run/species.py:51-102): the aligner's m8 text -> per species the uniquely mapped reads
// and their aligned bases, and the reads whose best hits tie as a CSR of (species, aln) for species_assign.cpp.
//
//   upload    the text goes up chunk_bytes at a time (a multiple of 16) into ONE resident buffer; the newlines of a chunk are
//             counted (text_rows.h, per 16 bytes) while the next one is copied, so a line or a query that straddles two chunks is
//             nothing special: the scan and everything after it run over the whole file
//   fields    a lane takes a line: it walks the line in aligned 16-byte loads, keeps where fields 0, 1, 2, 3 and 11 begin and
//             end (fields are runs of non-blanks, str.split()), decodes pid / aln / score / qlen and hashes the query name.  A wave
//             is 64 neighbouring lines, a few KB of text it reads front to back.  A number is decoded here when one exact
//             integer and one multiply or divide by an exact power of ten give float() of it (at most 15 significant digits,
//             decimal exponent within +-22); any other spelling goes on a side list and the host's exact parser patches it in
//   lookup    the target's bytes are looked up in an open-addressing table of the marker genes (hash, then the bytes compared)
//   filter    pid < cutoff[marker] and float(aln) / qlen < aln_cov as the fp64 expressions the reference evaluates
//   group     the passing lines are sorted by the hash of their query name (the library's stable radix sort, 32 bits a call);
//             inside a run of equal keys a line's query is the FIRST line of the run with the same bytes -- the run is walked,
//             names are compared byte for byte, so a narrow hash (hash_bits) only makes the runs longer
//   best      the query's top score by an integer atomic max over the order-preserving image of the double, the lines that
//             equal it, their number; one such line: the species' counters (integer atomics); more: the CSR, queries in the
//             order of their first passing line, hits in line order
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstring>
#include <string>
#include <string_view>
#include <vector>

#include "text_numbers.h"
#include "text_rows.h"

struct midas_species_result {
  std::vector<int64_t> indptr;
  std::vector<int32_t> species, aln;
  // dump: the decoded lines
  std::vector<double> pid, score;
  std::vector<int32_t> l_aln, l_qlen, l_species, l_marker;
  std::vector<uint8_t> l_pass;
};

namespace midas {
namespace {

enum SpReason : uint32_t { kSpFields = 1, kSpTarget = 2, kSpQlen = 3, kSpAln = 4, kSpNumber = 5, kSpCutoff = 6, kSpScoreNan = 7 };

const char* sp_reason(uint32_t r) {
  switch (r) {
    case kSpFields: return "fewer than 12 fields";
    case kSpTarget: return "the target is not a marker gene of phyeco.fa with a row in phyeco.map";
    case kSpQlen: return "the query name does not end in _<length> with a length that is a non-zero 32-bit integer";
    case kSpAln: return "the alignment length is not a 32-bit integer";
    case kSpNumber: return "pid or score is not a number";
    case kSpCutoff: return "the target's marker family has no cutoff in phyeco.mapping_cutoffs";
    case kSpScoreNan: return "the score is nan";
  }
  return "bad line";
}

__host__ __device__ inline bool sp_space(unsigned c) { return c == ' ' || (c >= '\t' && c <= '\r') || (c >= 0x1c && c <= 0x1f); }

__host__ __device__ inline unsigned long long sp_mix(unsigned long long h) {      // (the finaliser of MurmurHash3: every bit of h reaches the low ones)
  h ^= h >> 33; h *= 0xFF51AFD7ED558CCDull; h ^= h >> 33; h *= 0xC4CEB9FE1A85EC53ull; h ^= h >> 33;
  return h;
}

__host__ __device__ inline unsigned long long sp_hash(const char* s, uint32_t n) {   // FNV-1a, then mixed
  unsigned long long h = 0xCBF29CE484222325ull;
  for (uint32_t k = 0; k < n; ++k) { h ^= (unsigned char)s[k]; h *= 0x100000001B3ull; }
  return sp_mix(h);
}

// int(text) for [sign] and up to nine digits
__host__ __device__ inline bool sp_i32_fast(const char* s, uint32_t n, int32_t* out) {
  uint32_t i = 0;
  bool neg = false;
  if (i < n && (s[i] == '+' || s[i] == '-')) { neg = s[i] == '-'; ++i; }
  if (i >= n || n - i > 9) return false;
  int32_t v = 0;
  for (; i < n; ++i) {
    if (s[i] < '0' || s[i] > '9') return false;
    v = v * 10 + (s[i] - '0');
  }
  *out = neg ? -v : v;
  return true;
}

struct SpLines {          // one entry a line
  uint32_t *q_off, *q_len, *t_off, *t_len;
  unsigned long long* qhash;
  double *pid, *score;
  int32_t *aln, *qlen, *species, *marker;
  uint32_t* pass;
};

__device__ __forceinline__ void sp_side(SideCell* side, uint32_t* side_n, uint32_t cap, uint32_t row, uint32_t slot, uint32_t off, uint32_t len) {
  const uint32_t k = atomicAdd(side_n, 1u);
  if (k < cap) side[k] = SideCell{row, slot, off, len};
}

__device__ __forceinline__ void sp_bad(unsigned long long* bad, long long line, uint32_t reason) {
  atomicMin(bad, ((unsigned long long)line << 8) | reason);
}

// text is padded with zero bytes to a multiple of 16; ends[k] = offset of the newline that closes line k
__global__ __launch_bounds__(256) void sp_fields_kernel(const char* text, const uint32_t* ends, long long lines, SpLines L, SideCell* side,
                                                        uint32_t* side_n, uint32_t side_cap, unsigned long long* bad) {
  const long long line = (long long)blockIdx.x * 256 + threadIdx.x;
  if (line >= lines) return;
  const uint32_t begin = line ? ends[line - 1] + 1 : 0u, end = ends[line];
  uint32_t s0 = 0, e0 = 0, s1 = 0, e1 = 0, s2 = 0, e2 = 0, s3 = 0, e3 = 0, s11 = 0, e11 = 0;
  int field = -1;
  bool in = false;
  const uint4* t16 = reinterpret_cast<const uint4*>(text);
  for (uint32_t a = begin & ~15u; a < end; a += 16) {
    const uint4 v = t16[a >> 4];
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int b = 0; b < 16; ++b) {
      const uint32_t pos = a + b;
      if (pos < begin || pos >= end) continue;
      const unsigned c = (w[b >> 2] >> (8 * (b & 3))) & 0xFFu;
      const bool blank = sp_space(c);
      if (!blank && !in) {
        in = true;
        ++field;
        if (field == 0) s0 = pos; else if (field == 1) s1 = pos; else if (field == 2) s2 = pos; else if (field == 3) s3 = pos;
        else if (field == 11) s11 = pos;
      } else if (blank && in) {
        in = false;
        if (field == 0) e0 = pos; else if (field == 1) e1 = pos; else if (field == 2) e2 = pos; else if (field == 3) e3 = pos;
        else if (field == 11) e11 = pos;
      }
    }
  }
  if (in) {
    if (field == 0) e0 = end; else if (field == 1) e1 = end; else if (field == 2) e2 = end; else if (field == 3) e3 = end;
    else if (field == 11) e11 = end;
  }
  L.species[line] = -1;
  L.marker[line] = -1;
  L.pass[line] = 0u;
  L.q_off[line] = s0; L.q_len[line] = e0 - s0;
  L.t_off[line] = s1; L.t_len[line] = e1 - s1;
  L.pid[line] = 0.0; L.score[line] = 0.0; L.aln[line] = 0; L.qlen[line] = 0; L.qhash[line] = 0ull;
  if (field < 11) { sp_bad(bad, line + 1, kSpFields); return; }
  double x;
  if (sp_f64_fast(text + s2, e2 - s2, &x)) L.pid[line] = x; else sp_side(side, side_n, side_cap, (uint32_t)line, 0u, s2, e2 - s2);
  if (sp_f64_fast(text + s11, e11 - s11, &x)) L.score[line] = x; else sp_side(side, side_n, side_cap, (uint32_t)line, 2u, s11, e11 - s11);
  int32_t iv;
  if (sp_i32_fast(text + s3, e3 - s3, &iv)) L.aln[line] = iv; else sp_side(side, side_n, side_cap, (uint32_t)line, 1u, s3, e3 - s3);
  uint32_t u = e0;                                   // qlen: the text after the query's last '_' (the whole name when it has none)
  while (u > s0 && text[u - 1] != '_') --u;
  if (sp_i32_fast(text + u, e0 - u, &iv)) L.qlen[line] = iv; else sp_side(side, side_n, side_cap, (uint32_t)line, 3u, u, e0 - u);
  L.qhash[line] = sp_hash(text + s0, e0 - s0);
}

struct SpGenes {          // the marker genes of phyeco.fa that have a row in phyeco.map
  const int32_t* slot;    // [table]: gene + 1, 0 = empty
  uint32_t mask;          // table - 1
  const char* names;
  const uint32_t* name_off;    // [genes + 1]
  const int32_t *species, *marker;
};

__global__ __launch_bounds__(256) void sp_lookup_kernel(const char* text, long long lines, SpLines L, SpGenes G, unsigned long long* bad) {
  const long long line = (long long)blockIdx.x * 256 + threadIdx.x;
  if (line >= lines) return;
  const uint32_t off = L.t_off[line], len = L.t_len[line];
  if (len == 0) return;                               // (a short line: reported by the field pass)
  const char* t = text + off;
  uint32_t at = (uint32_t)sp_hash(t, len) & G.mask;
  for (;;) {
    const int32_t g = G.slot[at];
    if (g == 0) { sp_bad(bad, line + 1, kSpTarget); return; }
    const uint32_t a = G.name_off[g - 1], b = G.name_off[g];
    if (b - a == len) {
      uint32_t k = 0;
      while (k < len && G.names[a + k] == t[k]) ++k;
      if (k == len) { L.species[line] = G.species[g - 1]; L.marker[line] = G.marker[g - 1]; return; }
    }
    at = (at + 1) & G.mask;                           // (the table is at most half full: an empty slot ends every probe)
  }
}

__global__ __launch_bounds__(256) void sp_patch_kernel(const uint32_t* row, const uint32_t* slot, const unsigned long long* val, long long n, SpLines L) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint32_t r = row[i];
  const unsigned long long v = val[i];
  switch (slot[i]) {
    case 0: L.pid[r] = __longlong_as_double((long long)v); break;
    case 2: L.score[r] = __longlong_as_double((long long)v); break;
    case 1: L.aln[r] = (int32_t)(uint32_t)v; break;
    default: L.qlen[r] = (int32_t)(uint32_t)v; break;
  }
}

__global__ __launch_bounds__(256) void sp_filter_kernel(long long lines, SpLines L, const double* cutoff, double aln_cov, unsigned long long* bad) {
  const long long line = (long long)blockIdx.x * 256 + threadIdx.x;
  if (line >= lines) return;
  const int32_t mk = L.marker[line];
  if (mk < 0) return;                                 // (already reported)
  if (L.qlen[line] == 0) { sp_bad(bad, line + 1, kSpQlen); return; }
  const double c = cutoff[mk], score = L.score[line];
  if (c != c) { sp_bad(bad, line + 1, kSpCutoff); return; }
  if (score != score) { sp_bad(bad, line + 1, kSpScoreNan); return; }
  L.score[line] = score + 0.0;                        // (-0.0 equals 0.0 in the reference's comparisons: one image for both)
  const bool drop = L.pid[line] < c || (double)L.aln[line] / (double)L.qlen[line] < aln_cov;
  L.pass[line] = drop ? 0u : 1u;
}

// pass_at = exclusive scan of pass: the passing lines in line order, and the low word of their key
__global__ __launch_bounds__(256) void sp_compact_kernel(long long lines, const uint32_t* pass, const uint32_t* pass_at, const unsigned long long* qhash,
                                                         unsigned long long mask, uint32_t* pline, uint32_t* key, uint32_t* val) {
  const long long line = (long long)blockIdx.x * 256 + threadIdx.x;
  if (line >= lines || !pass[line]) return;
  const uint32_t p = pass_at[line];
  pline[p] = (uint32_t)line;
  key[p] = (uint32_t)(qhash[line] & mask);
  val[p] = p;
}

__global__ __launch_bounds__(256) void sp_key_hi_kernel(long long P, const uint32_t* val, const uint32_t* pline, const unsigned long long* qhash,
                                                        unsigned long long mask, uint32_t* key) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < P) key[i] = (uint32_t)((qhash[pline[val[i]]] & mask) >> 32);
}

__device__ __forceinline__ unsigned long long sp_ordered(double x) {      // a < b  <=>  sp_ordered(a) < sp_ordered(b), no nan
  const unsigned long long u = (unsigned long long)__double_as_longlong(x);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

// sv = the passing lines sorted by key, line order inside a key.  rep[p] = the first passing line (as a passing index) of p's query
__global__ __launch_bounds__(256) void sp_rep_kernel(const char* text, long long P, const uint32_t* sv, const uint32_t* pline, SpLines L,
                                                     unsigned long long mask, uint32_t* rep, unsigned long long* qmax) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= P) return;
  const uint32_t p = sv[i], line = pline[p];
  const unsigned long long h = L.qhash[line], key = h & mask;
  const uint32_t off = L.q_off[line], len = L.q_len[line];
  uint32_t first = p;
  for (long long j = i - 1; j >= 0; --j) {
    const uint32_t pj = sv[j], lj = pline[pj];
    const unsigned long long hj = L.qhash[lj];
    if ((hj & mask) != key) break;
    if (hj != h || L.q_len[lj] != len) continue;
    const uint32_t oj = L.q_off[lj];
    uint32_t k = 0;
    while (k < len && text[oj + k] == text[off + k]) ++k;
    if (k == len) first = pj;
  }
  rep[p] = first;
  atomicMax(&qmax[first], sp_ordered(L.score[line]));
}

__global__ __launch_bounds__(256) void sp_best_kernel(long long P, const uint32_t* pline, SpLines L, const uint32_t* rep, const unsigned long long* qmax,
                                                      uint32_t* best, uint32_t* nbest) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= P) return;
  const bool b = sp_ordered(L.score[pline[p]]) == qmax[rep[p]];
  best[p] = b ? 1u : 0u;
  if (b) atomicAdd(&nbest[rep[p]], 1u);
}

// a query with one best hit: its species' counters.  A query with more: its head p carries the number of hits
__global__ __launch_bounds__(256) void sp_unique_kernel(long long P, const uint32_t* pline, SpLines L, const uint32_t* rep, const uint32_t* best,
                                                        const uint32_t* nbest, unsigned long long* uniq_reads, unsigned long long* uniq_aln,
                                                        uint32_t* head_flag, uint32_t* head_size) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= P) return;
  const uint32_t n = nbest[rep[p]];
  const bool head = rep[p] == (uint32_t)p && n > 1;
  head_flag[p] = head ? 1u : 0u;
  head_size[p] = head ? n : 0u;
  if (best[p] && n == 1) {
    const uint32_t line = pline[p];
    atomicAdd(&uniq_reads[L.species[line]], 1ull);
    atomicAdd(&uniq_aln[L.species[line]], (unsigned long long)(long long)L.aln[line]);
  }
}

// the CSR: query head_at[rep] holds nbest[rep] hits from hit_at[rep] on; a hit's place among them is the number of best hits of
// its query in front of it in the sorted run (line order)
__global__ __launch_bounds__(256) void sp_csr_kernel(long long P, const uint32_t* sv, const uint32_t* pline, SpLines L, unsigned long long mask,
                                                     const uint32_t* rep, const uint32_t* best, const uint32_t* nbest, const uint32_t* head_at,
                                                     const uint32_t* hit_at, uint32_t* sizes, int32_t* hit_species, int32_t* hit_aln) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= P) return;
  const uint32_t p = sv[i], r = rep[p], n = nbest[r];
  if (n < 2) return;
  if (r == p) sizes[head_at[p]] = n;
  if (!best[p]) return;
  const uint32_t line = pline[p];
  const unsigned long long key = L.qhash[line] & mask;
  uint32_t rank = 0;
  for (long long j = i - 1; j >= 0; --j) {
    const uint32_t pj = sv[j];
    if ((L.qhash[pline[pj]] & mask) != key) break;
    rank += (rep[pj] == r && best[pj]) ? 1u : 0u;
  }
  hit_species[hit_at[r] + rank] = L.species[line];
  hit_aln[hit_at[r] + rank] = L.aln[line];
}

double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

}  // namespace
}  // namespace midas

using namespace midas;

extern "C" int32_t midas_species_parse_number(int32_t kind, const char* text, int64_t n, void* out, int32_t* out_fast) {
  if (!text || n < 0 || n > 0x7FFFFFFF || !out) return MIDAS_SNPS_ERR_INVALID_ARG;
  if (out_fast) *out_fast = 0;
  if (kind == 0) {
    double x = 0.0;
    if (sp_f64_fast(text, (uint32_t)n, &x)) { if (out_fast) *out_fast = 1; }
    else if (!parse_f64_py(std::string_view(text, (size_t)n), &x)) return MIDAS_SNPS_ERR_BAD_LAYOUT;
    *static_cast<double*>(out) = x;
    return MIDAS_SNPS_OK;
  }
  if (kind == 1) {
    int32_t v = 0;
    int64_t w = 0;
    if (sp_i32_fast(text, (uint32_t)n, &v)) { w = v; if (out_fast) *out_fast = 1; }
    else if (!parse_i64_py(std::string_view(text, (size_t)n), &w)) return MIDAS_SNPS_ERR_BAD_LAYOUT;
    *static_cast<int64_t*>(out) = w;
    return MIDAS_SNPS_OK;
  }
  return MIDAS_SNPS_ERR_INVALID_ARG;
}

extern "C" void midas_species_result_close(midas_species_result* r) { delete r; }

extern "C" int32_t midas_species_result_columns(const midas_species_result* r, int64_t* indptr, int32_t* species, int32_t* aln) {
  if (!r || !indptr) return MIDAS_SNPS_ERR_INVALID_ARG;
  std::memcpy(indptr, r->indptr.data(), r->indptr.size() * 8);
  if (!r->species.empty()) {
    if (!species || !aln) return MIDAS_SNPS_ERR_INVALID_ARG;
    std::memcpy(species, r->species.data(), r->species.size() * 4);
    std::memcpy(aln, r->aln.data(), r->aln.size() * 4);
  }
  return MIDAS_SNPS_OK;
}

extern "C" int32_t midas_species_result_lines(const midas_species_result* r, double* pid, double* score, int32_t* aln, int32_t* qlen, int32_t* species,
                                              int32_t* marker, uint8_t* pass) {
  if (!r) return MIDAS_SNPS_ERR_INVALID_ARG;
  const size_t n = r->l_pass.size();
  if (n == 0) return MIDAS_SNPS_OK;
  if (!pid || !score || !aln || !qlen || !species || !marker || !pass) return MIDAS_SNPS_ERR_INVALID_ARG;
  std::memcpy(pid, r->pid.data(), n * 8); std::memcpy(score, r->score.data(), n * 8);
  std::memcpy(aln, r->l_aln.data(), n * 4); std::memcpy(qlen, r->l_qlen.data(), n * 4);
  std::memcpy(species, r->l_species.data(), n * 4); std::memcpy(marker, r->l_marker.data(), n * 4);
  std::memcpy(pass, r->l_pass.data(), n);
  return MIDAS_SNPS_OK;
}

extern "C" int32_t midas_species_classify(midas_snps_ctx* ctx, const char* text, int64_t text_bytes, int32_t n_genes, const char* gene_names,
                                          const int64_t* gene_name_off, const int32_t* gene_species, const int32_t* gene_marker, int32_t n_species,
                                          int32_t n_markers, const double* marker_cutoff, double aln_cov, const int64_t* iparams4,
                                          int64_t* out_uniq_reads, int64_t* out_uniq_aln, int64_t* out_stats16, float* out_ms8,
                                          midas_species_result** out_result) {
  if (!ctx || text_bytes < 0 || (text_bytes > 0 && !text) || n_genes < 0 || n_species < 0 || n_markers < 0 || !iparams4 || !out_stats16 ||
      !out_result || (n_genes > 0 && (!gene_names || !gene_name_off || !gene_species || !gene_marker)) || (n_markers > 0 && !marker_cutoff) ||
      (n_species > 0 && (!out_uniq_reads || !out_uniq_aln)) || iparams4[0] < 0 || iparams4[1] < 0 || iparams4[1] > 64)
    return MIDAS_SNPS_ERR_INVALID_ARG;
  for (int32_t g = 0; g < n_genes; ++g)
    if (gene_species[g] < 0 || gene_species[g] >= n_species || gene_marker[g] < 0 || gene_marker[g] >= n_markers || gene_name_off[g + 1] < gene_name_off[g] ||
        gene_name_off[g] < 0 || gene_name_off[g + 1] > 0x7FFFFFFF)
      return MIDAS_SNPS_ERR_INVALID_ARG;
  ctx->clear_error();
  ctx->err_read = -1;
  *out_result = nullptr;
  for (int k = 0; k < 16; ++k) out_stats16[k] = 0;
  if (out_ms8) for (int k = 0; k < 8; ++k) out_ms8[k] = 0.f;
  for (int32_t s = 0; s < n_species; ++s) { out_uniq_reads[s] = 0; out_uniq_aln[s] = 0; }
  const bool dump = iparams4[2] != 0;
  const int hash_bits = iparams4[1] == 0 ? 64 : (int)iparams4[1];
  const unsigned long long mask = hash_bits >= 64 ? ~0ull : ((1ull << hash_bits) - 1);
  std::unique_ptr<midas_species_result> res(new midas_species_result);
  res->indptr.assign(1, 0);
  if (text_bytes == 0) { *out_result = res.release(); return MIDAS_SNPS_OK; }
  if (text_bytes > 0xFFFFFF00ll) return ss_fail(ctx, MIDAS_SNPS_ERR_UNSUPPORTED, "an alignment file beyond 4 GiB: line offsets are 32 bits");
  long long chunk_bytes = iparams4[0] == 0 ? (64ll << 20) : iparams4[0];
  chunk_bytes = std::max<long long>(64, (chunk_bytes + 15) / 16 * 16);
  SS_TRY(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  SsBufs dev;
  double ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};          // upload (+ newline counts), index, fields, lookup, filter + sort + group, best hits, download, -
  double t0 = now_ms();
  // ---- upload: the whole text stays resident -----------------------------------------------------------------------------------
  const bool add_nl = text[text_bytes - 1] != '\n';
  const long long n = text_bytes + (add_nl ? 1 : 0), n16 = (n + 15) / 16;
  char* d_text = nullptr;
  uint32_t *d_counts = nullptr, *d_scratch = nullptr;
  SS_TRY(dev.get(&d_text, (size_t)n16 * 16));
  SS_TRY(dev.get(&d_counts, ((size_t)n16 + 1) * 4));
  long long chunks = 0;
  for (long long at = 0; at < text_bytes; at += chunk_bytes, ++chunks) {
    const long long nb = std::min(chunk_bytes, text_bytes - at);
    SS_TRY(hipMemcpyAsync(d_text + at, text + at, (size_t)nb, hipMemcpyHostToDevice, st));
    long long w0 = at / 16, w1 = (at + nb) / 16;       // the 16-byte words this chunk completes
    if (at + nb == text_bytes) {
      if (add_nl) { static const char kNl = '\n'; SS_TRY(hipMemcpyAsync(d_text + text_bytes, &kNl, 1, hipMemcpyHostToDevice, st)); }
      if (n16 * 16 > n) SS_TRY(hipMemsetAsync(d_text + n, 0, (size_t)(n16 * 16 - n), st));
      w1 = n16;
    }
    if (w1 > w0) {
      hipLaunchKernelGGL(ss_count_kernel, dim3(nblocks(w1 - w0, 256)), dim3(256), 0, st, (const uint4*)d_text + w0, w1 - w0, d_counts + w0);
      SS_TRY(hipGetLastError());
    }
  }
  SS_TRY(hipMemsetAsync(d_counts + n16, 0, 4, st));
  SS_TRY(hipStreamSynchronize(st));
  ms[0] = now_ms() - t0; t0 = now_ms();
  // ---- the line index ------------------------------------------------------------------------------------------------------------
  SS_TRY(dev.get(&d_scratch, scan_scratch_words(n16 + 1) * 4));
  SS_TRY(launch_scan_u32(d_counts, d_counts, n16 + 1, d_scratch, st));
  uint32_t lines32 = 0;
  SS_TRY(hipMemcpyAsync(&lines32, d_counts + n16, 4, hipMemcpyDeviceToHost, st));
  SS_TRY(hipStreamSynchronize(st));
  const long long lines = lines32;
  if (lines > 0x7FFFFF00ll) return ss_fail(ctx, MIDAS_SNPS_ERR_UNSUPPORTED, "more than 2^31 alignment lines in one file");
  uint32_t* d_ends = nullptr;
  SS_TRY(dev.get(&d_ends, (size_t)lines * 4));
  hipLaunchKernelGGL(ss_ends_kernel, dim3(nblocks(n16, 256)), dim3(256), 0, st, (const uint4*)d_text, n16, d_counts, (uint32_t)lines, d_ends);
  SS_TRY(hipGetLastError());
  SS_TRY(hipStreamSynchronize(st));
  ms[1] = now_ms() - t0; t0 = now_ms();
  out_stats16[0] = lines;
  out_stats16[7] = chunks;
  out_stats16[8] = chunk_bytes;
  // ---- fields --------------------------------------------------------------------------------------------------------------------
  SpLines L{};
  const size_t nl = (size_t)lines;
  SS_TRY(dev.get(&L.q_off, nl * 4)); SS_TRY(dev.get(&L.q_len, nl * 4)); SS_TRY(dev.get(&L.t_off, nl * 4)); SS_TRY(dev.get(&L.t_len, nl * 4));
  SS_TRY(dev.get(&L.qhash, nl * 8)); SS_TRY(dev.get(&L.pid, nl * 8)); SS_TRY(dev.get(&L.score, nl * 8));
  SS_TRY(dev.get(&L.aln, nl * 4)); SS_TRY(dev.get(&L.qlen, nl * 4)); SS_TRY(dev.get(&L.species, nl * 4)); SS_TRY(dev.get(&L.marker, nl * 4));
  SS_TRY(dev.get(&L.pass, (nl + 1) * 4));
  unsigned long long* d_bad = nullptr;
  uint32_t* d_side_n = nullptr;
  SS_TRY(dev.get(&d_bad, 8));
  SS_TRY(dev.get(&d_side_n, 4));
  SS_TRY(hipMemsetAsync(d_bad, 0xFF, 8, st));
  uint32_t side_cap = (uint32_t)std::min<size_t>(nl / 8 + 1024, 0x7FFFFFFFu), side_n = 0;
  SideCell* d_side = nullptr;
  std::vector<SideCell> side;
  for (int round = 0; round < 2; ++round) {
    SS_TRY(dev.get(&d_side, (size_t)side_cap * sizeof(SideCell)));
    SS_TRY(hipMemsetAsync(d_side_n, 0, 4, st));
    hipLaunchKernelGGL(sp_fields_kernel, dim3(nblocks(lines, 256)), dim3(256), 0, st, d_text, d_ends, lines, L, d_side, d_side_n, side_cap, d_bad);
    SS_TRY(hipGetLastError());
    SS_TRY(hipMemcpyAsync(&side_n, d_side_n, 4, hipMemcpyDeviceToHost, st));
    SS_TRY(hipStreamSynchronize(st));
    if (side_n <= side_cap) break;
    side_cap = side_n;                                // (every line has at most four cells: the second round always fits)
  }
  out_stats16[6] = side_n;
  unsigned long long host_bad = kNoBad;
  if (side_n > 0) {                                   // the spellings the device leaves to the exact parser
    side.resize(side_n);
    SS_TRY(hipMemcpy(side.data(), d_side, (size_t)side_n * sizeof(SideCell), hipMemcpyDeviceToHost));
    std::vector<uint32_t> prow(side_n), pslot(side_n);
    std::vector<unsigned long long> pval(side_n);
    for (uint32_t k = 0; k < side_n; ++k) {
      const SideCell& c = side[k];
      const std::string_view v(text + c.off, c.len);
      prow[k] = c.row; pslot[k] = c.slot; pval[k] = 0;
      uint32_t why = 0;
      if (c.slot == 0 || c.slot == 2) {
        double x = 0.0;
        if (parse_f64_py(v, &x)) std::memcpy(&pval[k], &x, 8); else why = kSpNumber;
      } else {
        int64_t w = 0;
        if (parse_i64_py(v, &w) && w >= INT32_MIN && w <= INT32_MAX) pval[k] = (uint32_t)(int32_t)w; else why = c.slot == 1 ? kSpAln : kSpQlen;
      }
      if (why) host_bad = std::min(host_bad, ((unsigned long long)(c.row + 1ull) << 8) | why);
    }
    uint32_t *d_prow = nullptr, *d_pslot = nullptr;
    unsigned long long* d_pval = nullptr;
    SS_TRY(dev.get(&d_prow, (size_t)side_n * 4)); SS_TRY(dev.get(&d_pslot, (size_t)side_n * 4)); SS_TRY(dev.get(&d_pval, (size_t)side_n * 8));
    SS_TRY(hipMemcpy(d_prow, prow.data(), (size_t)side_n * 4, hipMemcpyHostToDevice));
    SS_TRY(hipMemcpy(d_pslot, pslot.data(), (size_t)side_n * 4, hipMemcpyHostToDevice));
    SS_TRY(hipMemcpy(d_pval, pval.data(), (size_t)side_n * 8, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(sp_patch_kernel, dim3(nblocks(side_n, 256)), dim3(256), 0, st, d_prow, d_pslot, d_pval, (long long)side_n, L);
    SS_TRY(hipGetLastError());
    SS_TRY(hipStreamSynchronize(st));
  }
  ms[2] = now_ms() - t0; t0 = now_ms();
  // ---- lookup --------------------------------------------------------------------------------------------------------------------
  SpGenes G{};
  {
    uint32_t table = 16;
    while (table < 2u * (uint32_t)n_genes + 2u) table <<= 1;
    std::vector<int32_t> slot(table, 0);
    std::vector<uint32_t> off((size_t)n_genes + 1, 0);
    const int64_t base = n_genes ? gene_name_off[0] : 0;
    for (int32_t g = 0; g <= n_genes && n_genes; ++g) off[g] = (uint32_t)(gene_name_off[g] - base);
    for (int32_t g = 0; g < n_genes; ++g) {
      const char* nm = gene_names + gene_name_off[g];
      const uint32_t len = off[g + 1] - off[g];
      uint32_t at = (uint32_t)sp_hash(nm, len) & (table - 1);
      bool twice = false;
      while (slot[at]) {                              // (a name listed twice: the later row stands, as in the reference's dict)
        const int32_t o = slot[at] - 1;
        if (off[o + 1] - off[o] == len && std::memcmp(gene_names + gene_name_off[o], nm, len) == 0) { twice = true; break; }
        at = (at + 1) & (table - 1);
      }
      (void)twice;
      slot[at] = g + 1;
    }
    int32_t *d_slot = nullptr, *d_gs = nullptr, *d_gm = nullptr;
    char* d_names = nullptr;
    uint32_t* d_off = nullptr;
    const size_t name_bytes = n_genes ? (size_t)(gene_name_off[n_genes] - base) : 0;
    SS_TRY(dev.get(&d_slot, (size_t)table * 4)); SS_TRY(dev.get(&d_gs, (size_t)n_genes * 4)); SS_TRY(dev.get(&d_gm, (size_t)n_genes * 4));
    SS_TRY(dev.get(&d_names, name_bytes)); SS_TRY(dev.get(&d_off, ((size_t)n_genes + 1) * 4));
    SS_TRY(hipMemcpy(d_slot, slot.data(), (size_t)table * 4, hipMemcpyHostToDevice));
    SS_TRY(hipMemcpy(d_off, off.data(), ((size_t)n_genes + 1) * 4, hipMemcpyHostToDevice));
    if (n_genes) {
      SS_TRY(hipMemcpy(d_gs, gene_species, (size_t)n_genes * 4, hipMemcpyHostToDevice));
      SS_TRY(hipMemcpy(d_gm, gene_marker, (size_t)n_genes * 4, hipMemcpyHostToDevice));
      if (name_bytes) SS_TRY(hipMemcpy(d_names, gene_names + base, name_bytes, hipMemcpyHostToDevice));
    }
    G.slot = d_slot; G.mask = table - 1; G.names = d_names; G.name_off = d_off; G.species = d_gs; G.marker = d_gm;
  }
  hipLaunchKernelGGL(sp_lookup_kernel, dim3(nblocks(lines, 256)), dim3(256), 0, st, d_text, lines, L, G, d_bad);
  SS_TRY(hipGetLastError());
  SS_TRY(hipStreamSynchronize(st));
  ms[3] = now_ms() - t0; t0 = now_ms();
  // ---- filter, then the first bad line of the file, whichever pass found it ----------------------------------------------------------
  double* d_cutoff = nullptr;
  SS_TRY(dev.get(&d_cutoff, (size_t)n_markers * 8));
  if (n_markers) SS_TRY(hipMemcpy(d_cutoff, marker_cutoff, (size_t)n_markers * 8, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(sp_filter_kernel, dim3(nblocks(lines, 256)), dim3(256), 0, st, lines, L, d_cutoff, aln_cov, d_bad);
  SS_TRY(hipGetLastError());
  unsigned long long bad = kNoBad;
  SS_TRY(hipMemcpyAsync(&bad, d_bad, 8, hipMemcpyDeviceToHost, st));
  SS_TRY(hipStreamSynchronize(st));
  bad = std::min(bad, host_bad);
  if (bad != kNoBad) {
    out_stats16[4] = (int64_t)(bad & 0xFFu);
    out_stats16[5] = (int64_t)(bad >> 8);
    ctx->err_read = (long long)(bad >> 8);
    char msg[256];
    snprintf(msg, sizeof msg, "alignments line %lld: %s", (long long)(bad >> 8), sp_reason((uint32_t)(bad & 0xFFu)));
    return ss_fail(ctx, MIDAS_SNPS_ERR_BAD_LAYOUT, msg);
  }
  // ---- the passing lines, sorted by the hash of their query ---------------------------------------------------------------------------
  uint32_t* d_pass_at = nullptr;
  SS_TRY(dev.get(&d_pass_at, (nl + 1) * 4));
  SS_TRY(hipMemsetAsync(L.pass + lines, 0, 4, st));
  uint32_t* d_scratch_lines = nullptr;
  SS_TRY(dev.get(&d_scratch_lines, scan_scratch_words(lines + 1) * 4));
  SS_TRY(launch_scan_u32(L.pass, d_pass_at, lines + 1, d_scratch_lines, st));
  uint32_t P32 = 0;
  SS_TRY(hipMemcpyAsync(&P32, d_pass_at + lines, 4, hipMemcpyDeviceToHost, st));
  SS_TRY(hipStreamSynchronize(st));
  const long long P = P32;
  out_stats16[1] = P;
  long long n_amb = 0, n_hits = 0;
  if (P > 0) {
    const size_t np = (size_t)P;
    uint32_t *d_pline = nullptr, *ka = nullptr, *va = nullptr, *kb = nullptr, *vb = nullptr, *d_sort = nullptr, *ks = nullptr, *sv = nullptr;
    SS_TRY(dev.get(&d_pline, np * 4)); SS_TRY(dev.get(&ka, np * 4)); SS_TRY(dev.get(&va, np * 4)); SS_TRY(dev.get(&kb, np * 4)); SS_TRY(dev.get(&vb, np * 4));
    SS_TRY(dev.get(&d_sort, std::max(sort_scratch_words(P), scan_scratch_words(P + 1)) * 4));
    hipLaunchKernelGGL(sp_compact_kernel, dim3(nblocks(lines, 256)), dim3(256), 0, st, lines, L.pass, d_pass_at, L.qhash, mask, d_pline, ka, va);
    SS_TRY(hipGetLastError());
    SS_TRY(launch_sort_pairs_u32(ka, va, kb, vb, P, std::min(hash_bits, 32), d_sort, st, &ks, &sv));
    if (hash_bits > 32) {
      uint32_t* ko = ks == ka ? kb : ka;
      uint32_t* vo = sv == va ? vb : va;
      hipLaunchKernelGGL(sp_key_hi_kernel, dim3(nblocks(P, 256)), dim3(256), 0, st, P, sv, d_pline, L.qhash, mask, ks);
      SS_TRY(hipGetLastError());
      SS_TRY(launch_sort_pairs_u32(ks, sv, ko, vo, P, hash_bits - 32, d_sort, st, &ks, &sv));
    }
    uint32_t *d_rep = nullptr, *d_best = nullptr, *d_nbest = nullptr, *d_flag = nullptr, *d_size = nullptr, *d_head_at = nullptr, *d_hit_at = nullptr;
    unsigned long long *d_qmax = nullptr, *d_ur = nullptr, *d_ua = nullptr;
    SS_TRY(dev.get(&d_rep, np * 4)); SS_TRY(dev.get(&d_best, np * 4)); SS_TRY(dev.get(&d_nbest, np * 4));
    SS_TRY(dev.get(&d_flag, (np + 1) * 4)); SS_TRY(dev.get(&d_size, (np + 1) * 4)); SS_TRY(dev.get(&d_head_at, (np + 1) * 4)); SS_TRY(dev.get(&d_hit_at, (np + 1) * 4));
    SS_TRY(dev.get(&d_qmax, np * 8)); SS_TRY(dev.get(&d_ur, (size_t)n_species * 8)); SS_TRY(dev.get(&d_ua, (size_t)n_species * 8));
    SS_TRY(hipMemsetAsync(d_qmax, 0, np * 8, st));
    SS_TRY(hipMemsetAsync(d_nbest, 0, np * 4, st));
    if (n_species) { SS_TRY(hipMemsetAsync(d_ur, 0, (size_t)n_species * 8, st)); SS_TRY(hipMemsetAsync(d_ua, 0, (size_t)n_species * 8, st)); }
    hipLaunchKernelGGL(sp_rep_kernel, dim3(nblocks(P, 256)), dim3(256), 0, st, d_text, P, sv, d_pline, L, mask, d_rep, d_qmax);
    SS_TRY(hipGetLastError());
    SS_TRY(hipStreamSynchronize(st));
    ms[4] = now_ms() - t0; t0 = now_ms();
    // ---- best hits ---------------------------------------------------------------------------------------------------------------
    hipLaunchKernelGGL(sp_best_kernel, dim3(nblocks(P, 256)), dim3(256), 0, st, P, d_pline, L, d_rep, d_qmax, d_best, d_nbest);
    SS_TRY(hipGetLastError());
    hipLaunchKernelGGL(sp_unique_kernel, dim3(nblocks(P, 256)), dim3(256), 0, st, P, d_pline, L, d_rep, d_best, d_nbest, d_ur, d_ua, d_flag, d_size);
    SS_TRY(hipGetLastError());
    SS_TRY(hipMemsetAsync(d_flag + P, 0, 4, st));
    SS_TRY(hipMemsetAsync(d_size + P, 0, 4, st));
    SS_TRY(launch_scan_u32(d_flag, d_head_at, P + 1, d_sort, st));
    SS_TRY(launch_scan_u32(d_size, d_hit_at, P + 1, d_sort, st));
    uint32_t tot[2] = {0, 0};
    SS_TRY(hipMemcpyAsync(&tot[0], d_head_at + P, 4, hipMemcpyDeviceToHost, st));
    SS_TRY(hipMemcpyAsync(&tot[1], d_hit_at + P, 4, hipMemcpyDeviceToHost, st));
    SS_TRY(hipStreamSynchronize(st));
    n_amb = tot[0];
    n_hits = tot[1];
    uint32_t* d_sizes = nullptr;
    int32_t *d_hs = nullptr, *d_ha = nullptr;
    SS_TRY(dev.get(&d_sizes, (size_t)n_amb * 4)); SS_TRY(dev.get(&d_hs, (size_t)n_hits * 4)); SS_TRY(dev.get(&d_ha, (size_t)n_hits * 4));
    hipLaunchKernelGGL(sp_csr_kernel, dim3(nblocks(P, 256)), dim3(256), 0, st, P, sv, d_pline, L, mask, d_rep, d_best, d_nbest, d_head_at, d_hit_at,
                       d_sizes, d_hs, d_ha);
    SS_TRY(hipGetLastError());
    SS_TRY(hipStreamSynchronize(st));
    ms[5] = now_ms() - t0; t0 = now_ms();
    // ---- download ----------------------------------------------------------------------------------------------------------------
    std::vector<uint32_t> sizes((size_t)n_amb);
    res->species.resize((size_t)n_hits);
    res->aln.resize((size_t)n_hits);
    if (n_amb) {
      SS_TRY(hipMemcpy(sizes.data(), d_sizes, (size_t)n_amb * 4, hipMemcpyDeviceToHost));
      SS_TRY(hipMemcpy(res->species.data(), d_hs, (size_t)n_hits * 4, hipMemcpyDeviceToHost));
      SS_TRY(hipMemcpy(res->aln.data(), d_ha, (size_t)n_hits * 4, hipMemcpyDeviceToHost));
    }
    res->indptr.resize((size_t)n_amb + 1);
    for (long long q = 0; q < n_amb; ++q) res->indptr[q + 1] = res->indptr[q] + sizes[q];
    if (n_species) {
      SS_TRY(hipMemcpy(out_uniq_reads, d_ur, (size_t)n_species * 8, hipMemcpyDeviceToHost));
      SS_TRY(hipMemcpy(out_uniq_aln, d_ua, (size_t)n_species * 8, hipMemcpyDeviceToHost));
    }
  }
  long long n_unique = 0;
  for (int32_t s = 0; s < n_species; ++s) n_unique += out_uniq_reads[s];
  out_stats16[2] = n_unique;
  out_stats16[3] = n_amb;
  out_stats16[9] = n_hits;
  if (dump) {
    res->pid.resize(nl); res->score.resize(nl); res->l_aln.resize(nl); res->l_qlen.resize(nl); res->l_species.resize(nl); res->l_marker.resize(nl);
    res->l_pass.resize(nl);
    std::vector<uint32_t> pass(nl);
    if (nl) {
      SS_TRY(hipMemcpy(res->pid.data(), L.pid, nl * 8, hipMemcpyDeviceToHost)); SS_TRY(hipMemcpy(res->score.data(), L.score, nl * 8, hipMemcpyDeviceToHost));
      SS_TRY(hipMemcpy(res->l_aln.data(), L.aln, nl * 4, hipMemcpyDeviceToHost)); SS_TRY(hipMemcpy(res->l_qlen.data(), L.qlen, nl * 4, hipMemcpyDeviceToHost));
      SS_TRY(hipMemcpy(res->l_species.data(), L.species, nl * 4, hipMemcpyDeviceToHost));
      SS_TRY(hipMemcpy(res->l_marker.data(), L.marker, nl * 4, hipMemcpyDeviceToHost));
      SS_TRY(hipMemcpy(pass.data(), L.pass, nl * 4, hipMemcpyDeviceToHost));
    }
    for (size_t k = 0; k < nl; ++k) res->l_pass[k] = (uint8_t)pass[k];
  }
  ms[6] = now_ms() - t0;
  if (out_ms8) for (int k = 0; k < 8; ++k) out_ms8[k] = (float)ms[k];
  *out_result = res.release();
  return MIDAS_SNPS_OK;
}
