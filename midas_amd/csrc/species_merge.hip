// merge_species.py (midas/merge/species.py): the samples' species/species_profile.txt -> three [species][sample] matrices
// (coverage, relative abundance fp64, count_reads int64) and per species the mean and median of the first two over the
// samples, its prevalence and its rank in species_prevalence.txt.
//
//   read + upload   host threads read GROUPS OF WHOLE FILES (at most chunk_bytes of text; a larger file is a group by itself)
//                   into one of two pinned buffers, every file closed by a '\n' of ours, and the group goes up into a device
//                   buffer that is reused; group g + 1 is read while group g is on the device.  Only the matrices stay resident
//   index           newlines counted per 16 bytes, the library's scan, ends[k] (text_rows.h); a file's first line is the number
//                   of newlines in front of it; a lane per file reads its header: where the four named columns stand (the last
//                   of equal names, as dict(zip()) keeps it) and how many fields a line must have
//   fields          a lane takes a line, 64 neighbouring lines a wave: aligned 16-byte loads, tabs counted, the four columns
//                   kept; a line whose field count is not the header's is skipped.  The doubles by the exact one-multiply path
//                   of text_rows.h, the integer up to 18 digits; any other spelling goes on the side list, the host's exact
//                   parser converts it and a patch kernel puts it in
//   lookup          the species id's bytes in an open-addressing table of species_info.txt's ids (hash, then the bytes);
//                   seen[species][sample] = the lowest line of the profile that names the species (atomicMin)
//   scatter         the line that seen names writes its three values at [species][sample]; any other line is a species twice
//   completeness    after the last group: a cell of seen still unset is a species missing from a profile
//   statistics      a workgroup per species row: numpy's pairwise add-reduce and one divide for the two means, the prevalence
//                   count, and for rows up to lds_bound samples a bitonic sort of the order-preserving integer image in LDS
//                   for the two medians.  Longer rows: the library's stable radix sort over (species, image), 32 bits a call.
//                   round(x, 2) of a numpy double is rint(x * 100) / 100 (this file is compiled with -ffp-contract=off)
//   order           stable radix sort of the species by n_samples - prevalence: the rows of species_prevalence.txt
//
// The first bad line is an atomicMin over (sample, line, reason); a missing species counts as the line after its profile's last.
#include <hip/hip_runtime.h>

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <atomic>
#include <charconv>
#include <chrono>
#include <cmath>
#include <cstring>
#include <future>
#include <string>
#include <string_view>
#include <vector>

#include "species_table.h"
#include "text_numbers.h"
#include "text_rows.h"
#include "workers.h"

struct midas_species_merge_result {
  int32_t n_species = 0, n_samples = 0;
  std::string ids;
  std::vector<int64_t> id_off;
  std::vector<double> coverage, abundance;      // [species][sample]
  std::vector<int64_t> reads;
  std::vector<double> stats;                    // [8][species]: mean_coverage, median_coverage, mean_abundance, median_abundance, then the four rounded
  std::vector<int64_t> prevalence;
  std::vector<int32_t> order;                   // the species of row k of species_prevalence.txt
};

namespace midas {
namespace {

enum SmReason : uint32_t {
  kSmHeaderId = 1, kSmHeaderReads = 2, kSmHeaderCov = 3, kSmHeaderAb = 4,      // the header lacks this column
  kSmUnknown = 5, kSmTwice = 6, kSmCellReads = 7, kSmCellCov = 8, kSmCellAb = 9, kSmNonFiniteCov = 10, kSmNonFiniteAb = 11, kSmReadsRange = 12,
  kSmMissing = 13
};

const char* const kSmColumn[4] = {"species_id", "count_reads", "coverage", "relative_abundance"};

// int(text) for [sign] and up to 18 digits
__host__ __device__ inline bool sm_i64_fast(const char* s, uint32_t n, long long* out) {
  uint32_t i = 0;
  bool neg = false;
  if (i < n && (s[i] == '+' || s[i] == '-')) { neg = s[i] == '-'; ++i; }
  if (i >= n || n - i > 18) return false;
  long long v = 0;
  for (; i < n; ++i) {
    if (s[i] < '0' || s[i] > '9') return false;
    v = v * 10 + (s[i] - '0');
  }
  *out = neg ? -v : v;
  return true;
}

__device__ __forceinline__ void sm_bad(unsigned long long* bad, uint32_t sample, uint32_t line, uint32_t reason) {
  atomicMin(bad, ((unsigned long long)sample << 40) | ((unsigned long long)line << 8) | reason);
}

// line0[f] = the group's line that is file f's header, f <= files (ends are sorted: the newlines in front of file_off[f])
__global__ __launch_bounds__(256) void sm_file_lines_kernel(const uint32_t* ends, uint32_t lines, const uint32_t* file_off, int files, uint32_t* line0) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f > files) return;
  const uint32_t at = file_off[f];
  uint32_t lo = 0, hi = lines;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (ends[mid] < at) lo = mid + 1; else hi = mid;
  }
  line0[f] = lo;
}

// cols[4 f + k] = the field of file f's header that is column k (the last one of that name), fields[f] = its number of fields
__global__ __launch_bounds__(64) void sm_header_kernel(const char* text, const uint32_t* ends, const uint32_t* file_off, const uint32_t* line0, int files,
                                                       uint32_t sample0, int32_t* cols, uint32_t* fields, unsigned long long* bad) {
  const int f = blockIdx.x * 64 + threadIdx.x;
  if (f >= files) return;
  const char* const names[4] = {"species_id", "count_reads", "coverage", "relative_abundance"};
  const uint32_t lens[4] = {10, 11, 8, 18};
  const uint32_t begin = file_off[f], end = ends[line0[f]];
  int32_t c[4] = {-1, -1, -1, -1};
  uint32_t field = 0, fs = begin;
  for (uint32_t pos = begin; pos <= end; ++pos) {
    if (pos < end && text[pos] != '\t') continue;
    for (int k = 0; k < 4; ++k) {
      if (pos - fs != lens[k]) continue;
      uint32_t j = 0;
      while (j < lens[k] && text[fs + j] == names[k][j]) ++j;
      if (j == lens[k]) c[k] = (int32_t)field;
    }
    ++field;
    fs = pos + 1;
  }
  fields[f] = field;
  for (int k = 0; k < 4; ++k) cols[4 * f + k] = c[k];
  for (int k = 0; k < 4; ++k)
    if (c[k] < 0) { sm_bad(bad, sample0 + (uint32_t)f, 1u, kSmHeaderId + (uint32_t)k); break; }
}

struct SmLines {          // one entry a line of the group
  uint32_t *file, *id_off, *id_len, *live;
  double *cov, *ab;
  long long* reads;
  int32_t* species;
};

// text is padded with zero bytes to a multiple of 16; ends[k] = offset of the newline that closes line k
__global__ __launch_bounds__(256) void sm_fields_kernel(const char* text, const uint32_t* ends, long long lines, const uint32_t* line0, int files,
                                                        const int32_t* cols, const uint32_t* fields, SmLines L, SideCell* side, uint32_t* side_n,
                                                        uint32_t side_cap) {
  const long long line = (long long)blockIdx.x * 256 + threadIdx.x;
  if (line >= lines) return;
  int lo = 0, hi = files;                                // the file: the last f with line0[f] <= line
  while (hi - lo > 1) {
    const int mid = (lo + hi) / 2;
    if (line0[mid] <= (uint32_t)line) lo = mid; else hi = mid;
  }
  const int f = lo;
  L.file[line] = (uint32_t)f;
  L.live[line] = 0u;
  L.species[line] = -1;
  L.id_off[line] = 0u; L.id_len[line] = 0u;
  L.cov[line] = 0.0; L.ab[line] = 0.0; L.reads[line] = 0;
  if (line0[f] == (uint32_t)line) return;                // the header
  const int32_t c0 = cols[4 * f], c1 = cols[4 * f + 1], c2 = cols[4 * f + 2], c3 = cols[4 * f + 3];
  if (c0 < 0 || c1 < 0 || c2 < 0 || c3 < 0) return;      // (reported by the header pass)
  const uint32_t begin = ends[line - 1] + 1, end = ends[line];
  uint32_t s[4] = {0, 0, 0, 0}, e[4] = {0, 0, 0, 0};
  int32_t field = 0;
  uint32_t fs = begin;
  const uint4* t16 = reinterpret_cast<const uint4*>(text);
  for (uint32_t a = begin & ~15u; a < end; a += 16) {
    const uint4 v = t16[a >> 4];
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int b = 0; b < 16; ++b) {
      const uint32_t pos = a + b;
      if (pos < begin || pos >= end) continue;
      if (((w[b >> 2] >> (8 * (b & 3))) & 0xFFu) != '\t') continue;
      if (field == c0) { s[0] = fs; e[0] = pos; }
      if (field == c1) { s[1] = fs; e[1] = pos; }
      if (field == c2) { s[2] = fs; e[2] = pos; }
      if (field == c3) { s[3] = fs; e[3] = pos; }
      ++field;
      fs = pos + 1;
    }
  }
  if (field == c0) { s[0] = fs; e[0] = end; }
  if (field == c1) { s[1] = fs; e[1] = end; }
  if (field == c2) { s[2] = fs; e[2] = end; }
  if (field == c3) { s[3] = fs; e[3] = end; }
  if ((uint32_t)(field + 1) != fields[f]) return;        // utility.parse_file drops the line
  L.live[line] = 1u;
  L.id_off[line] = s[0]; L.id_len[line] = e[0] - s[0];
  long long iv;
  double x;
  if (sm_i64_fast(text + s[1], e[1] - s[1], &iv)) L.reads[line] = iv;
  else { const uint32_t k = atomicAdd(side_n, 1u); if (k < side_cap) side[k] = SideCell{(uint32_t)line, 0u, s[1], e[1] - s[1]}; }
  if (sp_f64_fast(text + s[2], e[2] - s[2], &x)) L.cov[line] = x;
  else { const uint32_t k = atomicAdd(side_n, 1u); if (k < side_cap) side[k] = SideCell{(uint32_t)line, 1u, s[2], e[2] - s[2]}; }
  if (sp_f64_fast(text + s[3], e[3] - s[3], &x)) L.ab[line] = x;
  else { const uint32_t k = atomicAdd(side_n, 1u); if (k < side_cap) side[k] = SideCell{(uint32_t)line, 2u, s[3], e[3] - s[3]}; }
}

__global__ __launch_bounds__(256) void sm_patch_kernel(const uint32_t* row, const uint32_t* slot, const unsigned long long* val, long long n, SmLines L) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint32_t r = row[i];
  const long long v = (long long)val[i];
  if (slot[i] == 0) L.reads[r] = v;
  else if (slot[i] == 1) L.cov[r] = __longlong_as_double(v);
  else L.ab[r] = __longlong_as_double(v);
}

struct SmTable {          // the species ids of species_info.txt
  const int32_t* slot;    // [table]: species + 1, 0 = empty
  uint32_t mask;
  const char* names;
  const uint32_t* name_off;    // [species + 1]
};

__global__ __launch_bounds__(256) void sm_lookup_kernel(const char* text, long long lines, const uint32_t* line0, uint32_t sample0, long long S, SmLines L,
                                                        SmTable T, uint32_t* seen, unsigned long long* bad) {
  const long long line = (long long)blockIdx.x * 256 + threadIdx.x;
  if (line >= lines || !L.live[line]) return;
  const uint32_t f = L.file[line], in_file = (uint32_t)line - line0[f] + 1u;      // 1-based, the header is line 1
  const uint32_t len = L.id_len[line];
  const char* t = text + L.id_off[line];
  uint32_t at = (uint32_t)sm_hash(t, len) & T.mask;
  for (;;) {
    const int32_t g = T.slot[at];
    if (g == 0) { sm_bad(bad, sample0 + f, in_file, kSmUnknown); return; }
    const uint32_t a = T.name_off[g - 1], b = T.name_off[g];
    if (b - a == len) {
      uint32_t k = 0;
      while (k < len && T.names[a + k] == t[k]) ++k;
      if (k == len) {
        L.species[line] = g - 1;
        atomicMin(&seen[(long long)(g - 1) * S + sample0 + f], in_file);
        return;
      }
    }
    at = (at + 1) & T.mask;                            // (the table is at most half full: an empty slot ends every probe)
  }
}

__global__ __launch_bounds__(256) void sm_scatter_kernel(long long lines, const uint32_t* line0, uint32_t sample0, long long S, SmLines L, const uint32_t* seen,
                                                         double* cov, double* ab, long long* reads, unsigned long long* bad) {
  const long long line = (long long)blockIdx.x * 256 + threadIdx.x;
  if (line >= lines || !L.live[line]) return;
  const int32_t sp = L.species[line];
  if (sp < 0) return;
  const uint32_t f = L.file[line], in_file = (uint32_t)line - line0[f] + 1u;
  const long long at = (long long)sp * S + sample0 + f;
  if (seen[at] != in_file) { sm_bad(bad, sample0 + f, in_file, kSmTwice); return; }
  cov[at] = L.cov[line]; ab[at] = L.ab[line]; reads[at] = L.reads[line];
}

// the earliest (sample, species) below sample_limit that no line set
__global__ __launch_bounds__(256) void sm_missing_kernel(const uint32_t* seen, long long cells, long long S, long long sample_limit, unsigned long long* miss) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= cells) return;
  const long long sp = i / S, s = i % S;
  if (s < sample_limit && seen[i] == 0xFFFFFFFFu) atomicMin(miss, ((unsigned long long)s << 32) | (unsigned long long)sp);
}

// numpy's pairwise_sum over n <= 128 values (eight partial sums, then the tail), as sites_call.h forms it
__device__ double sm_pairwise_leaf(const double* a, long long n) {
  if (n < 8) {
    double res = 0.0;
    for (long long i = 0; i < n; ++i) res += a[i];
    return res;
  }
  double r[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) r[j] = a[j];
  long long i = 8;
  for (; i < n - (n % 8); i += 8) {
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] += a[i + j];
  }
  double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
  for (; i < n; ++i) res += a[i];
  return res;
}

// numpy's add.reduce of n values: halves cut at multiples of eight down to blocks of at most 128, left before right
__device__ double sm_pairwise_sum(const double* a, long long n) {
  struct Frame { long long at, n; double left; int st; };
  Frame stk[40];
  int sp = 0;
  stk[sp++] = Frame{0, n, 0.0, 0};
  double ret = 0.0;
  while (sp > 0) {
    Frame& f = stk[sp - 1];
    long long n2 = f.n / 2;
    n2 -= n2 % 8;
    if (f.st == 0) {
      if (f.n <= 128) {
        ret = sm_pairwise_leaf(a + f.at, f.n);
        --sp;
      } else {
        f.st = 1;
        stk[sp++] = Frame{f.at, n2, 0.0, 0};
      }
    } else if (f.st == 1) {
      f.left = ret;
      f.st = 2;
      stk[sp++] = Frame{f.at + n2, f.n - n2, 0.0, 0};
    } else {
      ret = f.left + ret;
      --sp;
    }
  }
  return ret;
}

__host__ __device__ inline unsigned long long sm_ordered(double x) {      // a < b  <=>  sm_ordered(a) < sm_ordered(b), no nan
  unsigned long long u;
  memcpy(&u, &x, 8);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

__device__ __forceinline__ double sm_unordered(unsigned long long k) {
  const unsigned long long u = (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k;
  return __longlong_as_double((long long)u);
}

// np.median of a row whose two middle values (equal for an odd count) are a <= b: np.mean of them, 0.0 + a [+ b] then one divide
__device__ __forceinline__ double sm_median(double a, double b, bool odd) { return odd ? (0.0 + a) / 1.0 : ((0.0 + a) + b) / 2.0; }

__device__ __forceinline__ double sm_round2(double x) { return rint(x * 100.0) / 100.0; }     // numpy's round(x, 2)

// a workgroup a species row.  n_pow2 > 0: the row is sorted in LDS (n_pow2 >= S keys, dynamic shared memory) and the medians
// are written; n_pow2 == 0: means and prevalence only, the medians come from the radix sort.  stats = [8][n_species]
__global__ __launch_bounds__(256) void sm_stats_kernel(const double* cov, const double* ab, int n_species, int S, int n_pow2, double depth, double* stats,
                                                       uint32_t* prevalence, uint32_t* order_key) {
  extern __shared__ unsigned long long sk[];
  __shared__ uint32_t prev;
  const int row = blockIdx.x, tid = threadIdx.x;
  const double* c = cov + (long long)row * S;
  const double* a = ab + (long long)row * S;
  if (tid == 0) prev = 0u;
  __syncthreads();
  uint32_t mine = 0;
  for (int i = tid; i < S; i += 256) mine += c[i] >= depth ? 1u : 0u;
  if (mine) atomicAdd(&prev, mine);
  if (tid == 0 || tid == 64) {                           // two waves, a mean each
    const int m = tid == 0 ? 0 : 2;
    // (np.mean starts its reduce from 0.0: a row of eight or more -0.0, whose pairwise sum is -0.0, has the mean 0.0)
    const double mean = __ddiv_rn(0.0 + sm_pairwise_sum(m == 0 ? c : a, S), (double)S);
    stats[(long long)m * n_species + row] = mean;
    stats[(long long)(m + 4) * n_species + row] = sm_round2(mean);
  }
  __syncthreads();
  if (tid == 0) { prevalence[row] = prev; order_key[row] = (uint32_t)S - prev; }
  if (n_pow2 == 0) return;
  for (int m = 0; m < 2; ++m) {
    const double* v = m == 0 ? c : a;
    for (int i = tid; i < n_pow2; i += 256) sk[i] = i < S ? sm_ordered(v[i]) : ~0ull;
    __syncthreads();
    for (int k = 2; k <= n_pow2; k <<= 1)
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int i = tid; i < n_pow2; i += 256) {
          const int o = i ^ j;
          if (o > i) {
            const unsigned long long x = sk[i], y = sk[o];
            if (((i & k) == 0) ? x > y : x < y) { sk[i] = y; sk[o] = x; }
          }
        }
        __syncthreads();
      }
    if (tid == 0) {
      const double med = sm_median(sm_unordered(sk[(S - 1) / 2]), sm_unordered(sk[S / 2]), S & 1);
      stats[(long long)(2 * m + 1) * n_species + row] = med;
      stats[(long long)(2 * m + 5) * n_species + row] = sm_round2(med);
    }
    __syncthreads();
  }
}

// the long rows: keys of the three radix passes over the cells of a matrix (low word of the image, high word, species)
__global__ __launch_bounds__(256) void sm_key_lo_kernel(const double* m, long long n, uint32_t* key, uint32_t* val) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  key[i] = (uint32_t)sm_ordered(m[i]);
  val[i] = (uint32_t)i;
}
__global__ __launch_bounds__(256) void sm_key_hi_kernel(const double* m, long long n, const uint32_t* val, uint32_t* key) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) key[i] = (uint32_t)(sm_ordered(m[val[i]]) >> 32);
}
__global__ __launch_bounds__(256) void sm_key_row_kernel(long long n, uint32_t S, const uint32_t* val, uint32_t* key) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) key[i] = val[i] / S;
}
// val = the cells sorted by (species, image): row r lies at [r S, (r + 1) S)
__global__ __launch_bounds__(256) void sm_long_median_kernel(const double* m, const uint32_t* val, int n_species, int S, int which, double* stats) {
  const int row = blockIdx.x * 256 + threadIdx.x;
  if (row >= n_species) return;
  const long long base = (long long)row * S;
  const double med = sm_median(m[val[base + (S - 1) / 2]], m[val[base + S / 2]], S & 1);
  stats[(long long)(2 * which + 1) * n_species + row] = med;
  stats[(long long)(2 * which + 5) * n_species + row] = sm_round2(med);
}
__global__ __launch_bounds__(256) void sm_iota_kernel(long long n, uint32_t* val) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) val[i] = (uint32_t)i;
}

double sm_now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

struct SmGrow {           // a device buffer that is reused and only ever grows
  void* p = nullptr;
  size_t cap = 0;
  ~SmGrow() { if (p) (void)hipFree(p); }
  hipError_t need(size_t bytes) {
    if (bytes <= cap && p) return hipSuccess;
    if (p) (void)hipFree(p);
    p = nullptr; cap = 0;
    const size_t want = std::max<size_t>(bytes + bytes / 4, 256);
    const hipError_t e = hipMalloc(&p, want);
    if (e == hipSuccess) cap = want;
    return e;
  }
  template <class T> T* as() { return static_cast<T*>(p); }
};

struct SmPinned {
  char* p = nullptr;
  size_t cap = 0;
  ~SmPinned() { if (p) (void)hipHostFree(p); }
  hipError_t need(size_t bytes) {
    if (bytes <= cap && p) return hipSuccess;
    if (p) (void)hipHostFree(p);
    p = nullptr; cap = 0;
    void* q = nullptr;
    const hipError_t e = hipHostMalloc(&q, bytes, hipHostMallocDefault);
    if (e == hipSuccess) { p = static_cast<char*>(q); cap = bytes; }
    return e;
  }
};

struct SmGroup { int32_t first = 0, files = 0; long long bytes = 0; };      // samples [first, first + files), their text with a '\n' each

// the files of a group into buf (file k at off[k], closed by '\n'); "" or what went wrong.  *own_newline counts the files that
// ended in '\n' by themselves: ours then closes an empty line more, which is no line of the file
std::string sm_read_group(const char* const* paths, const std::vector<long long>& size, const SmGroup& g, const std::vector<uint32_t>& off, char* buf,
                          int threads, std::atomic<long long>* own_newline) {
  std::atomic<int> next{0};
  std::mutex m;
  std::string err;
  Workers::run(std::max(1, std::min(threads, g.files)), [&] {
    for (int k; (k = next.fetch_add(1)) < g.files;) {
      const int s = g.first + k;
      const long long want = size[(size_t)s];
      char* to = buf + off[(size_t)k];
      std::string why;
      const int fd = open(paths[s], O_RDONLY);
      if (fd < 0) {
        why = "cannot read";
      } else {
        long long got = 0;
        while (got < want) {
          const ssize_t r = pread(fd, to + got, (size_t)(want - got), (off_t)got);
          if (r <= 0) break;
          got += r;
        }
        char extra;
        if (got != want || pread(fd, &extra, 1, (off_t)want) > 0) why = "changed while it was read";
        close(fd);
      }
      to[want] = '\n';
      if (why.empty() && want > 0 && to[want - 1] == '\n') own_newline->fetch_add(1);
      if (!why.empty()) {
        std::lock_guard<std::mutex> lock(m);
        if (err.empty()) err = std::string(paths[s]) + ": " + why;
      }
    }
  });
  return err;
}

}  // namespace
}  // namespace midas

using namespace midas;

extern "C" void midas_species_merge_result_close(midas_species_merge_result* r) { delete r; }

extern "C" int32_t midas_species_merge_result_matrices(const midas_species_merge_result* r, double* coverage, double* abundance, int64_t* reads) {
  if (!r) return MIDAS_SNPS_ERR_INVALID_ARG;
  const size_t n = r->coverage.size();
  if (n == 0) return MIDAS_SNPS_OK;
  if (!coverage || !abundance || !reads) return MIDAS_SNPS_ERR_INVALID_ARG;
  std::memcpy(coverage, r->coverage.data(), n * 8);
  std::memcpy(abundance, r->abundance.data(), n * 8);
  std::memcpy(reads, r->reads.data(), n * 8);
  return MIDAS_SNPS_OK;
}

extern "C" int32_t midas_species_merge_result_stats(const midas_species_merge_result* r, double* stats8, int64_t* prevalence, int32_t* order) {
  if (!r) return MIDAS_SNPS_ERR_INVALID_ARG;
  const size_t n = (size_t)r->n_species;
  if (n == 0) return MIDAS_SNPS_OK;
  if (!stats8 || !prevalence || !order) return MIDAS_SNPS_ERR_INVALID_ARG;
  std::memcpy(stats8, r->stats.data(), 8 * n * 8);
  std::memcpy(prevalence, r->prevalence.data(), n * 8);
  std::memcpy(order, r->order.data(), n * 4);
  return MIDAS_SNPS_OK;
}

// relative_abundance.txt, coverage.txt, count_reads.txt and species_prevalence.txt into outdir
extern "C" int32_t midas_species_merge_result_write(const midas_species_merge_result* r, const char* outdir, const char* header_line, int32_t threads,
                                                    char* err1024) {
  if (!r || !outdir || !header_line) return MIDAS_SNPS_ERR_INVALID_ARG;
  const int64_t R = r->n_species, S = r->n_samples;
  const int nt = std::max(1, threads > 0 ? threads : cpu_budget());
  const char* const names[3] = {"relative_abundance", "coverage", "count_reads"};
  for (int kind = 0; kind < 3; ++kind) {
    const std::string path = std::string(outdir) + "/" + names[kind] + ".txt";
    FILE* f = fopen(path.c_str(), "wb");
    bool ok = f && fputs(header_line, f) >= 0;
    const double* vf = kind == 0 ? r->abundance.data() : r->coverage.data();
    const int64_t block = std::max<int64_t>(1, 65536 / std::max<int64_t>(1, S)), n_blocks = (R + block - 1) / block, wave = (int64_t)nt * 4;
    std::vector<std::string> text;
    for (int64_t b0 = 0; b0 < n_blocks && ok; b0 += wave) {       // row blocks formatted in parallel, written in order
      const int64_t nb = std::min(wave, n_blocks - b0);
      text.assign((size_t)nb, std::string());
      std::atomic<int64_t> next{0};
      Workers::run((int)std::min<int64_t>(nt, nb), [&] {
        std::vector<char> cells((size_t)(33 * S + 1));
        for (int64_t k; (k = next.fetch_add(1)) < nb;) {
          std::string& s = text[(size_t)k];
          const int64_t r0 = (b0 + k) * block, r1 = std::min(R, r0 + block);
          for (int64_t row = r0; row < r1; ++row) {
            s.append(r->ids.data() + r->id_off[(size_t)row], (size_t)(r->id_off[(size_t)row + 1] - r->id_off[(size_t)row]));
            if (kind < 2) {                                   // repr of the S doubles, '\n' after each: the separators become tabs
              int64_t len = 0;
              midas_genes_merge_format_f64(S, vf + row * S, cells.data(), (int64_t)cells.size(), &len);
              for (int64_t j = 0; j < len; ++j)
                if (cells[(size_t)j] == '\n') cells[(size_t)j] = '\t';
              if (len > 0) { s.push_back('\t'); s.append(cells.data(), (size_t)len - 1); }
            } else {
              char cell[24];
              for (int64_t j = 0; j < S; ++j) {
                s.push_back('\t');
                s.append(cell, (size_t)(std::to_chars(cell, cell + 24, r->reads[(size_t)(row * S + j)]).ptr - cell));
              }
            }
            s.push_back('\n');
          }
        }
      });
      for (const auto& s : text)
        if (fwrite(s.data(), 1, s.size(), f) != s.size()) { ok = false; break; }
    }
    if (f && fclose(f) != 0) ok = false;
    if (!ok) {
      if (err1024) snprintf(err1024, 1024, "cannot write %.900s", path.c_str());
      return MIDAS_SNPS_ERR_INVALID_ARG;
    }
  }
  const std::string path = std::string(outdir) + "/species_prevalence.txt";
  FILE* f = fopen(path.c_str(), "wb");
  bool ok = f && fputs("species_id\tmean_coverage\tmedian_coverage\tmean_abundance\tmedian_abundance\tprevalence\n", f) >= 0;
  std::string s;
  char cells[4 * 33 + 1], cell[24];
  for (int64_t k = 0; k < R && ok; ++k) {
    const int64_t row = r->order[(size_t)k];
    double v[4];
    for (int j = 0; j < 4; ++j) v[j] = r->stats[(size_t)((4 + j) * R + row)];
    int64_t len = 0;
    midas_genes_merge_format_f64(4, v, cells, (int64_t)sizeof cells, &len);
    for (int64_t j = 0; j < len; ++j)
      if (cells[j] == '\n') cells[j] = '\t';
    s.assign(r->ids.data() + r->id_off[(size_t)row], (size_t)(r->id_off[(size_t)row + 1] - r->id_off[(size_t)row]));
    s.push_back('\t');
    s.append(cells, (size_t)len);
    s.append(cell, (size_t)(std::to_chars(cell, cell + 24, r->prevalence[(size_t)row]).ptr - cell));
    s.push_back('\n');
    ok = fwrite(s.data(), 1, s.size(), f) == s.size();
  }
  if (f && fclose(f) != 0) ok = false;
  if (!ok) {
    if (err1024) snprintf(err1024, 1024, "cannot write %.900s", path.c_str());
    return MIDAS_SNPS_ERR_INVALID_ARG;
  }
  return MIDAS_SNPS_OK;
}

extern "C" int32_t midas_species_merge(midas_snps_ctx* ctx, int32_t n_samples, const char* const* profile_paths, int32_t n_species, const char* species_ids,
                                       const int64_t* species_id_off, double sample_depth, const int64_t* iparams4, int64_t* out_stats16, float* out_ms8,
                                       midas_species_merge_result** out_result) {
  if (!ctx || n_samples <= 0 || n_samples >= (1 << 24) || !profile_paths || n_species <= 0 || !species_ids || !species_id_off || !iparams4 || !out_stats16 ||
      !out_result || iparams4[0] < 0 || iparams4[1] < 0 || iparams4[2] < 0 || sample_depth != sample_depth)
    return MIDAS_SNPS_ERR_INVALID_ARG;
  for (int32_t g = 0; g < n_species; ++g)
    if (species_id_off[g] < 0 || species_id_off[g + 1] < species_id_off[g] || species_id_off[g + 1] - species_id_off[0] > 0x7FFFFFFF) return MIDAS_SNPS_ERR_INVALID_ARG;
  ctx->clear_error();
  ctx->err_read = -1;
  *out_result = nullptr;
  for (int k = 0; k < 16; ++k) out_stats16[k] = 0;
  if (out_ms8) for (int k = 0; k < 8; ++k) out_ms8[k] = 0.f;
  const long long S = n_samples, R = n_species, cells = S * R;
  long long chunk_bytes = iparams4[0] == 0 ? (256ll << 20) : iparams4[0];
  const int lds_bound = (int)std::min<long long>(iparams4[1] == 0 ? 4096 : iparams4[1], 4096);
  const int threads = iparams4[2] > 0 ? (int)std::min<long long>(iparams4[2], 256) : cpu_budget();
  double ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};          // read, upload, index, fields, lookup + scatter, statistics, download, -
  // ---- the table of species ids (duplicates are the caller's to drop) ---------------------------------------------------------------
  const int64_t id_base = species_id_off[0];
  std::vector<uint32_t> name_off((size_t)R + 1);
  for (long long g = 0; g <= R; ++g) name_off[(size_t)g] = (uint32_t)(species_id_off[g] - id_base);
  std::vector<int32_t> slot;
  if (!species_table_build(species_ids, species_id_off, n_species, &slot)) return ss_fail(ctx, MIDAS_SNPS_ERR_INVALID_ARG, "a species id is listed twice");
  const uint32_t table = (uint32_t)slot.size();
  // ---- the groups of whole files ----------------------------------------------------------------------------------------------------
  std::vector<long long> size((size_t)S);
  for (long long s = 0; s < S; ++s) {
    struct stat sb;
    if (!profile_paths[s] || stat(profile_paths[s], &sb) != 0 || !S_ISREG(sb.st_mode))
      return ss_fail(ctx, MIDAS_SNPS_ERR_INVALID_ARG, (std::string("cannot read ") + (profile_paths[s] ? profile_paths[s] : "(null)")).c_str());
    size[(size_t)s] = (long long)sb.st_size;
    if (size[(size_t)s] + 1 > 0xFFFFFF00ll) return ss_fail(ctx, MIDAS_SNPS_ERR_UNSUPPORTED, "a species profile beyond 4 GiB: text offsets are 32 bits");
  }
  chunk_bytes = std::min<long long>(std::max<long long>(chunk_bytes, 16), 0xFFFFFF00ll);
  std::vector<SmGroup> groups;
  long long max_bytes = 0, max_files = 0, total_bytes = 0;
  for (long long s = 0; s < S; ++s) {
    const long long b = size[(size_t)s] + 1;
    if (groups.empty() || groups.back().bytes + b > chunk_bytes) groups.push_back(SmGroup{(int32_t)s, 0, 0});
    groups.back().files += 1;
    groups.back().bytes += b;
    total_bytes += b;
  }
  for (const SmGroup& g : groups) { max_bytes = std::max(max_bytes, g.bytes); max_files = std::max<long long>(max_files, g.files); }
  SS_TRY(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  // ---- room: the matrices are checked against what the device has free before anything is allocated -----------------------------------
  {
    size_t free_b = 0, total_b = 0;
    SS_TRY(hipMemGetInfo(&free_b, &total_b));
    const double want = (double)cells * 28.0 + (double)max_bytes * 2.0;
    if (want > (double)free_b * 0.9) {
      char msg[256];
      snprintf(msg, sizeof msg, "%lld species x %lld samples need %.1f GB of device memory for the matrices, %.1f GB are free", R, S, want / 1e9,
               (double)free_b / 1e9);
      return ss_fail(ctx, MIDAS_SNPS_ERR_OUT_OF_MEMORY, msg);
    }
  }
  const bool long_rows = S > lds_bound;
  if (long_rows && cells > 0xFFFFFF00ll) return ss_fail(ctx, MIDAS_SNPS_ERR_UNSUPPORTED, "rows beyond the LDS bound with more than 2^32 cells in all");
  SsBufs dev;
  double *d_cov = nullptr, *d_ab = nullptr;
  long long* d_reads = nullptr;
  uint32_t* d_seen = nullptr;
  SS_TRY(dev.get(&d_cov, (size_t)cells * 8)); SS_TRY(dev.get(&d_ab, (size_t)cells * 8)); SS_TRY(dev.get(&d_reads, (size_t)cells * 8));
  SS_TRY(dev.get(&d_seen, (size_t)cells * 4));
  SS_TRY(hipMemsetAsync(d_cov, 0, (size_t)cells * 8, st)); SS_TRY(hipMemsetAsync(d_ab, 0, (size_t)cells * 8, st));
  SS_TRY(hipMemsetAsync(d_reads, 0, (size_t)cells * 8, st)); SS_TRY(hipMemsetAsync(d_seen, 0xFF, (size_t)cells * 4, st));
  SmTable T{};
  {
    int32_t* d_slot = nullptr;
    char* d_names = nullptr;
    uint32_t* d_off = nullptr;
    const size_t name_bytes = name_off[(size_t)R];
    SS_TRY(dev.get(&d_slot, (size_t)table * 4)); SS_TRY(dev.get(&d_names, name_bytes)); SS_TRY(dev.get(&d_off, ((size_t)R + 1) * 4));
    SS_TRY(hipMemcpy(d_slot, slot.data(), (size_t)table * 4, hipMemcpyHostToDevice));
    SS_TRY(hipMemcpy(d_off, name_off.data(), ((size_t)R + 1) * 4, hipMemcpyHostToDevice));
    if (name_bytes) SS_TRY(hipMemcpy(d_names, species_ids + id_base, name_bytes, hipMemcpyHostToDevice));
    T.slot = d_slot; T.mask = table - 1; T.names = d_names; T.name_off = d_off;
  }
  const size_t text_cap = ((size_t)max_bytes + 15) / 16 * 16;
  char* d_text = nullptr;
  uint32_t *d_counts = nullptr, *d_scratch = nullptr, *d_file_off = nullptr, *d_line0 = nullptr, *d_fields = nullptr, *d_side_n = nullptr;
  int32_t* d_cols = nullptr;
  unsigned long long* d_bad = nullptr;
  SS_TRY(dev.get(&d_text, text_cap));
  SS_TRY(dev.get(&d_counts, (text_cap / 16 + 1) * 4));
  SS_TRY(dev.get(&d_scratch, scan_scratch_words((long long)(text_cap / 16 + 1)) * 4));
  SS_TRY(dev.get(&d_file_off, ((size_t)max_files + 1) * 4)); SS_TRY(dev.get(&d_line0, ((size_t)max_files + 1) * 4));
  SS_TRY(dev.get(&d_fields, (size_t)max_files * 4)); SS_TRY(dev.get(&d_cols, (size_t)max_files * 16));
  SS_TRY(dev.get(&d_side_n, 4)); SS_TRY(dev.get(&d_bad, 16));
  SS_TRY(hipMemsetAsync(d_bad, 0xFF, 16, st));
  SmGrow g_ends, g_file, g_id_off, g_id_len, g_live, g_cov, g_ab, g_reads, g_species, g_side, g_prow, g_pslot, g_pval;
  SmPinned pinned[2];
  std::vector<std::vector<uint32_t>> file_off(2);
  auto lay_out = [&](size_t gi) {                         // where the files of group gi stand in its buffer
    const SmGroup& g = groups[gi];
    std::vector<uint32_t>& off = file_off[gi & 1];
    off.assign((size_t)g.files + 1, 0u);
    for (int k = 0; k < g.files; ++k) off[(size_t)k + 1] = off[(size_t)k] + (uint32_t)(size[(size_t)(g.first + k)] + 1);
  };
  double t0 = sm_now_ms();
  SS_TRY(pinned[0].need(text_cap));
  if (groups.size() > 1) SS_TRY(pinned[1].need(text_cap));
  lay_out(0);
  std::atomic<long long> own_newline{0};
  std::string read_err = sm_read_group(profile_paths, size, groups[0], file_off[0], pinned[0].p, threads, &own_newline);
  ms[0] += sm_now_ms() - t0;
  unsigned long long bad = kNoBad;
  std::string bad_id;
  long long total_lines = 0, total_side = 0;
  std::vector<uint32_t> line0;
  for (size_t gi = 0; gi < groups.size(); ++gi) {
    if (!read_err.empty()) return ss_fail(ctx, MIDAS_SNPS_ERR_INVALID_ARG, read_err.c_str());
    const SmGroup& g = groups[gi];
    const char* host = pinned[gi & 1].p;
    const std::vector<uint32_t>& off = file_off[gi & 1];
    std::future<std::string> ahead;                       // the next group is read while this one is on the device
    if (gi + 1 < groups.size()) {
      lay_out(gi + 1);
      ahead = std::async(std::launch::async, [&, gi] {
        return sm_read_group(profile_paths, size, groups[gi + 1], file_off[(gi + 1) & 1], pinned[(gi + 1) & 1].p, threads, &own_newline);
      });
    }
    struct Join {                                         // (no way out of this round leaves the reader running)
      std::future<std::string>& f;
      ~Join() { if (f.valid()) f.wait(); }
    } join{ahead};
    // ---- upload ---------------------------------------------------------------------------------------------------------------------
    t0 = sm_now_ms();
    const long long n = g.bytes, n16 = (n + 15) / 16;
    SS_TRY(hipMemcpyAsync(d_text, host, (size_t)n, hipMemcpyHostToDevice, st));
    if (n16 * 16 > n) SS_TRY(hipMemsetAsync(d_text + n, 0, (size_t)(n16 * 16 - n), st));
    SS_TRY(hipMemcpyAsync(d_file_off, off.data(), ((size_t)g.files + 1) * 4, hipMemcpyHostToDevice, st));
    SS_TRY(hipStreamSynchronize(st));
    ms[1] += sm_now_ms() - t0; t0 = sm_now_ms();
    // ---- the line index, the files' first lines, their headers ----------------------------------------------------------------------------
    hipLaunchKernelGGL(ss_count_kernel, dim3(nblocks(n16, 256)), dim3(256), 0, st, (const uint4*)d_text, n16, d_counts);
    SS_TRY(hipGetLastError());
    SS_TRY(hipMemsetAsync(d_counts + n16, 0, 4, st));
    SS_TRY(launch_scan_u32(d_counts, d_counts, n16 + 1, d_scratch, st));
    uint32_t lines32 = 0;
    SS_TRY(hipMemcpyAsync(&lines32, d_counts + n16, 4, hipMemcpyDeviceToHost, st));
    SS_TRY(hipStreamSynchronize(st));
    const long long lines = lines32;                      // (at least one a file: the '\n' that closes it)
    if (lines > 0x7FFFFF00ll) return ss_fail(ctx, MIDAS_SNPS_ERR_UNSUPPORTED, "more than 2^31 lines in one group of species profiles");
    const size_t nl = (size_t)lines;
    SS_TRY(g_ends.need(nl * 4));
    uint32_t* d_ends = g_ends.as<uint32_t>();
    hipLaunchKernelGGL(ss_ends_kernel, dim3(nblocks(n16, 256)), dim3(256), 0, st, (const uint4*)d_text, n16, d_counts, (uint32_t)lines, d_ends);
    SS_TRY(hipGetLastError());
    hipLaunchKernelGGL(sm_file_lines_kernel, dim3(nblocks(g.files + 1, 256)), dim3(256), 0, st, d_ends, (uint32_t)lines, d_file_off, g.files, d_line0);
    SS_TRY(hipGetLastError());
    hipLaunchKernelGGL(sm_header_kernel, dim3(nblocks(g.files, 64)), dim3(64), 0, st, d_text, d_ends, d_file_off, d_line0, g.files, (uint32_t)g.first, d_cols,
                       d_fields, d_bad);
    SS_TRY(hipGetLastError());
    line0.resize((size_t)g.files + 1);
    SS_TRY(hipMemcpyAsync(line0.data(), d_line0, ((size_t)g.files + 1) * 4, hipMemcpyDeviceToHost, st));
    SS_TRY(hipStreamSynchronize(st));
    ms[2] += sm_now_ms() - t0; t0 = sm_now_ms();
    total_lines += lines;
    // ---- fields ---------------------------------------------------------------------------------------------------------------------
    SmLines L{};
    SS_TRY(g_file.need(nl * 4)); SS_TRY(g_id_off.need(nl * 4)); SS_TRY(g_id_len.need(nl * 4)); SS_TRY(g_live.need(nl * 4));
    SS_TRY(g_cov.need(nl * 8)); SS_TRY(g_ab.need(nl * 8)); SS_TRY(g_reads.need(nl * 8)); SS_TRY(g_species.need(nl * 4));
    L.file = g_file.as<uint32_t>(); L.id_off = g_id_off.as<uint32_t>(); L.id_len = g_id_len.as<uint32_t>(); L.live = g_live.as<uint32_t>();
    L.cov = g_cov.as<double>(); L.ab = g_ab.as<double>(); L.reads = g_reads.as<long long>(); L.species = g_species.as<int32_t>();
    uint32_t side_cap = (uint32_t)std::min<size_t>(nl / 8 + 1024, 0x7FFFFFFFu), side_n = 0;
    for (int round = 0; round < 2; ++round) {
      SS_TRY(g_side.need((size_t)side_cap * sizeof(SideCell)));
      SS_TRY(hipMemsetAsync(d_side_n, 0, 4, st));
      hipLaunchKernelGGL(sm_fields_kernel, dim3(nblocks(lines, 256)), dim3(256), 0, st, d_text, d_ends, lines, d_line0, g.files, d_cols, d_fields, L,
                         g_side.as<SideCell>(), d_side_n, side_cap);
      SS_TRY(hipGetLastError());
      SS_TRY(hipMemcpyAsync(&side_n, d_side_n, 4, hipMemcpyDeviceToHost, st));
      SS_TRY(hipStreamSynchronize(st));
      if (side_n <= side_cap) break;
      if ((unsigned long long)side_n * sizeof(SideCell) > 0x7FFFFFFFull * 4) return ss_fail(ctx, MIDAS_SNPS_ERR_UNSUPPORTED, "too many cells for the host's parser");
      side_cap = side_n;                                  // (a line has at most three cells: the second round always fits)
    }
    total_side += side_n;
    unsigned long long host_bad = kNoBad;
    if (side_n > 0) {                                     // the spellings the device leaves to the exact parser
      std::vector<SideCell> side(side_n);
      SS_TRY(hipMemcpy(side.data(), g_side.p, (size_t)side_n * sizeof(SideCell), hipMemcpyDeviceToHost));
      std::vector<uint32_t> prow(side_n), pslot(side_n);
      std::vector<unsigned long long> pval(side_n);
      std::atomic<uint32_t> next{0};
      std::mutex bad_m;
      const uint32_t step = 4096;                        // (real profiles hold 16 and 17 digit doubles: millions of cells, parsed by all threads)
      Workers::run((int)std::max<uint32_t>(1u, std::min<uint32_t>((uint32_t)threads, (side_n + step - 1) / step)), [&] {
        unsigned long long mine = kNoBad;
        for (uint32_t k0; (k0 = next.fetch_add(step)) < side_n;)
          for (uint32_t k = k0; k < std::min(side_n, k0 + step); ++k) {
            const SideCell& c = side[k];
            const std::string_view v(host + c.off, c.len);
            prow[k] = c.row; pslot[k] = c.slot; pval[k] = 0;
            uint32_t why = 0;
            if (c.slot == 0) {
              int64_t w = 0;
              if (parse_i64_py(v, &w)) {
                std::memcpy(&pval[k], &w, 8);
              } else {                                    // digits (and separators) alone: an integer, but none of 64 bits
                std::string z;
                std::string_view d = trim(v);
                if (!d.empty() && (d[0] == '+' || d[0] == '-')) d.remove_prefix(1);
                const bool digits = strip_digit_separators(d, &z) && !z.empty() && z.find_first_not_of("0123456789") == std::string::npos;
                why = digits ? kSmReadsRange : kSmCellReads;
              }
            } else {
              double x = 0.0;
              if (!parse_f64_py(v, &x)) why = c.slot == 1 ? kSmCellCov : kSmCellAb;
              else if (!std::isfinite(x)) why = c.slot == 1 ? kSmNonFiniteCov : kSmNonFiniteAb;
              else std::memcpy(&pval[k], &x, 8);
            }
            if (why) {
              const uint32_t f = (uint32_t)(std::upper_bound(line0.begin(), line0.end() - 1, c.row) - line0.begin()) - 1u;
              mine = std::min(mine, ((unsigned long long)((uint32_t)g.first + f) << 40) | ((unsigned long long)(c.row - line0[f] + 1u) << 8) | why);
            }
          }
        std::lock_guard<std::mutex> lock(bad_m);
        host_bad = std::min(host_bad, mine);
      });
      SS_TRY(g_prow.need((size_t)side_n * 4)); SS_TRY(g_pslot.need((size_t)side_n * 4)); SS_TRY(g_pval.need((size_t)side_n * 8));
      SS_TRY(hipMemcpy(g_prow.p, prow.data(), (size_t)side_n * 4, hipMemcpyHostToDevice));
      SS_TRY(hipMemcpy(g_pslot.p, pslot.data(), (size_t)side_n * 4, hipMemcpyHostToDevice));
      SS_TRY(hipMemcpy(g_pval.p, pval.data(), (size_t)side_n * 8, hipMemcpyHostToDevice));
      hipLaunchKernelGGL(sm_patch_kernel, dim3(nblocks(side_n, 256)), dim3(256), 0, st, g_prow.as<uint32_t>(), g_pslot.as<uint32_t>(),
                         g_pval.as<unsigned long long>(), (long long)side_n, L);
      SS_TRY(hipGetLastError());
      SS_TRY(hipStreamSynchronize(st));
    }
    ms[3] += sm_now_ms() - t0; t0 = sm_now_ms();
    // ---- lookup + scatter -------------------------------------------------------------------------------------------------------------
    hipLaunchKernelGGL(sm_lookup_kernel, dim3(nblocks(lines, 256)), dim3(256), 0, st, d_text, lines, d_line0, (uint32_t)g.first, S, L, T, d_seen, d_bad);
    SS_TRY(hipGetLastError());
    hipLaunchKernelGGL(sm_scatter_kernel, dim3(nblocks(lines, 256)), dim3(256), 0, st, lines, d_line0, (uint32_t)g.first, S, L, d_seen, d_cov, d_ab, d_reads,
                       d_bad);
    SS_TRY(hipGetLastError());
    SS_TRY(hipMemcpyAsync(&bad, d_bad, 8, hipMemcpyDeviceToHost, st));
    SS_TRY(hipStreamSynchronize(st));
    ms[4] += sm_now_ms() - t0;
    bad = std::min(bad, host_bad);
    if (bad != kNoBad) {                                  // the earliest bad line lies in this group: its species id, for the message
      const uint32_t f = (uint32_t)(bad >> 40) - (uint32_t)g.first, row = line0[f] + (uint32_t)((bad >> 8) & 0xFFFFFFFFu) - 1u;
      uint32_t o = 0, len = 0;
      SS_TRY(hipMemcpy(&o, L.id_off + row, 4, hipMemcpyDeviceToHost));
      SS_TRY(hipMemcpy(&len, L.id_len + row, 4, hipMemcpyDeviceToHost));
      bad_id.assign(host + o, std::min<uint32_t>(len, 200u));
      break;
    }
    t0 = sm_now_ms();
    if (ahead.valid()) read_err = ahead.get();
    ms[0] += sm_now_ms() - t0;
  }
  out_stats16[0] = total_lines - own_newline.load();
  out_stats16[1] = (int64_t)groups.size();
  out_stats16[2] = chunk_bytes;
  out_stats16[3] = total_side;
  out_stats16[8] = long_rows ? 0 : 1;
  out_stats16[9] = lds_bound;
  out_stats16[11] = total_bytes;
  // ---- completeness: every (species, sample) in front of the first bad line ---------------------------------------------------------------
  {
    const long long limit = bad == kNoBad ? S : (long long)(bad >> 40);
    unsigned long long miss = kNoBad;
    hipLaunchKernelGGL(sm_missing_kernel, dim3(nblocks(cells, 256)), dim3(256), 0, st, d_seen, cells, S, limit, d_bad + 1);
    SS_TRY(hipGetLastError());
    SS_TRY(hipMemcpyAsync(&miss, d_bad + 1, 8, hipMemcpyDeviceToHost, st));
    SS_TRY(hipStreamSynchronize(st));
    char msg[1024];
    if (miss != kNoBad) {
      const long long s = (long long)(miss >> 32), sp = (long long)(miss & 0xFFFFFFFFu);
      out_stats16[4] = kSmMissing; out_stats16[5] = s; out_stats16[6] = 0; out_stats16[7] = sp;
      snprintf(msg, sizeof msg, "%.600s: species '%.200s' of species_info.txt has no line", profile_paths[s],
               std::string(species_ids + species_id_off[sp], (size_t)(species_id_off[sp + 1] - species_id_off[sp])).c_str());
      return ss_fail(ctx, MIDAS_SNPS_ERR_BAD_LAYOUT, msg);
    }
    if (bad != kNoBad) {
      const long long s = (long long)(bad >> 40), line = (long long)((bad >> 8) & 0xFFFFFFFFu);
      const uint32_t why = (uint32_t)(bad & 0xFFu);
      out_stats16[4] = why; out_stats16[5] = s; out_stats16[6] = line; out_stats16[7] = -1;
      ctx->err_read = line;
      if (why <= kSmHeaderAb) snprintf(msg, sizeof msg, "%.600s line 1: the header has no column '%s'", profile_paths[s], kSmColumn[why - 1]);
      else if (why == kSmUnknown) snprintf(msg, sizeof msg, "%.600s line %lld: species '%s' is not in species_info.txt", profile_paths[s], line, bad_id.c_str());
      else if (why == kSmTwice) snprintf(msg, sizeof msg, "%.600s line %lld: species '%s' stands on an earlier line too", profile_paths[s], line, bad_id.c_str());
      else if (why == kSmReadsRange) snprintf(msg, sizeof msg, "%.600s line %lld: count_reads of species '%s' is beyond 64 bits", profile_paths[s], line, bad_id.c_str());
      else if (why == kSmNonFiniteCov || why == kSmNonFiniteAb)
        snprintf(msg, sizeof msg, "%.600s line %lld: %s of species '%s' is not finite", profile_paths[s], line, kSmColumn[why == kSmNonFiniteCov ? 2 : 3], bad_id.c_str());
      else
        snprintf(msg, sizeof msg, "%.600s line %lld: %s of species '%s' is not a number", profile_paths[s], line, kSmColumn[why - kSmCellReads + 1], bad_id.c_str());
      return ss_fail(ctx, MIDAS_SNPS_ERR_BAD_LAYOUT, msg);
    }
  }
  // ---- row statistics, the order of species_prevalence.txt --------------------------------------------------------------------------------
  t0 = sm_now_ms();
  double* d_stats = nullptr;
  uint32_t *d_prev = nullptr, *ka = nullptr, *va = nullptr, *kb = nullptr, *vb = nullptr, *d_sort = nullptr, *ks = nullptr, *vs = nullptr;
  const long long n_sort = long_rows ? cells : R;
  SS_TRY(dev.get(&d_stats, (size_t)R * 64)); SS_TRY(dev.get(&d_prev, (size_t)R * 4));
  SS_TRY(dev.get(&ka, (size_t)n_sort * 4)); SS_TRY(dev.get(&va, (size_t)n_sort * 4)); SS_TRY(dev.get(&kb, (size_t)n_sort * 4)); SS_TRY(dev.get(&vb, (size_t)n_sort * 4));
  SS_TRY(dev.get(&d_sort, sort_scratch_words(n_sort) * 4));
  int n_pow2 = 0;
  if (!long_rows) { n_pow2 = 2; while (n_pow2 < S) n_pow2 <<= 1; }
  if (long_rows) {
    int row_bits = 1;
    while ((1ll << row_bits) < R) ++row_bits;
    for (int which = 0; which < 2; ++which) {
      const double* m = which == 0 ? d_cov : d_ab;
      hipLaunchKernelGGL(sm_key_lo_kernel, dim3(nblocks(cells, 256)), dim3(256), 0, st, m, cells, ka, va);
      SS_TRY(hipGetLastError());
      SS_TRY(launch_sort_pairs_u32(ka, va, kb, vb, cells, 32, d_sort, st, &ks, &vs));
      for (int pass = 0; pass < 2; ++pass) {
        uint32_t* ko = ks == ka ? kb : ka;
        uint32_t* vo = vs == va ? vb : va;
        if (pass == 0) hipLaunchKernelGGL(sm_key_hi_kernel, dim3(nblocks(cells, 256)), dim3(256), 0, st, m, cells, vs, ks);
        else hipLaunchKernelGGL(sm_key_row_kernel, dim3(nblocks(cells, 256)), dim3(256), 0, st, cells, (uint32_t)S, vs, ks);
        SS_TRY(hipGetLastError());
        SS_TRY(launch_sort_pairs_u32(ks, vs, ko, vo, cells, pass == 0 ? 32 : row_bits, d_sort, st, &ks, &vs));
      }
      hipLaunchKernelGGL(sm_long_median_kernel, dim3(nblocks(R, 256)), dim3(256), 0, st, m, vs, (int)R, (int)S, which, d_stats);
      SS_TRY(hipGetLastError());
    }
  }
  hipLaunchKernelGGL(sm_stats_kernel, dim3((unsigned)R), dim3(256), (size_t)n_pow2 * 8, st, d_cov, d_ab, (int)R, (int)S, n_pow2, sample_depth, d_stats, d_prev, ka);
  SS_TRY(hipGetLastError());
  int s_bits = 1;
  while ((1ll << s_bits) <= S) ++s_bits;
  hipLaunchKernelGGL(sm_iota_kernel, dim3(nblocks(R, 256)), dim3(256), 0, st, R, va);
  SS_TRY(hipGetLastError());
  SS_TRY(launch_sort_pairs_u32(ka, va, kb, vb, R, s_bits, d_sort, st, &ks, &vs));
  SS_TRY(hipStreamSynchronize(st));
  ms[5] = sm_now_ms() - t0; t0 = sm_now_ms();
  // ---- download ---------------------------------------------------------------------------------------------------------------------
  std::unique_ptr<midas_species_merge_result> res(new midas_species_merge_result);
  res->n_species = n_species; res->n_samples = n_samples;
  res->ids.assign(species_ids + id_base, name_off[(size_t)R]);
  res->id_off.assign(name_off.begin(), name_off.end());
  res->coverage.resize((size_t)cells); res->abundance.resize((size_t)cells); res->reads.resize((size_t)cells);
  res->stats.resize((size_t)R * 8); res->prevalence.resize((size_t)R); res->order.resize((size_t)R);
  std::vector<uint32_t> prev((size_t)R), order((size_t)R);
  SS_TRY(hipMemcpy(res->coverage.data(), d_cov, (size_t)cells * 8, hipMemcpyDeviceToHost));
  SS_TRY(hipMemcpy(res->abundance.data(), d_ab, (size_t)cells * 8, hipMemcpyDeviceToHost));
  SS_TRY(hipMemcpy(res->reads.data(), d_reads, (size_t)cells * 8, hipMemcpyDeviceToHost));
  SS_TRY(hipMemcpy(res->stats.data(), d_stats, (size_t)R * 64, hipMemcpyDeviceToHost));
  SS_TRY(hipMemcpy(prev.data(), d_prev, (size_t)R * 4, hipMemcpyDeviceToHost));
  SS_TRY(hipMemcpy(order.data(), vs, (size_t)R * 4, hipMemcpyDeviceToHost));
  for (long long k = 0; k < R; ++k) { res->prevalence[(size_t)k] = prev[(size_t)k]; res->order[(size_t)k] = (int32_t)order[(size_t)k]; }
  ms[6] = sm_now_ms() - t0;
  if (out_ms8) for (int k = 0; k < 8; ++k) out_ms8[k] = (float)ms[k];
  *out_result = res.release();
  return MIDAS_SNPS_OK;
}
