// The two generic device primitives this library needs, written for it (gfx950; no hipCUB / rocPRIM on the product path):
//   * an exclusive scan of 32-bit counters (three phases: sums of 4096, their scan by one workgroup, the scan applied);
//   * a STABLE least-significant-digit radix sort of (32-bit key, value) pairs, eight bits of the key a pass, for keys whose
//     range is known (a gene index, a tile bin): as many passes as the range has bytes.  Input order survives inside a key --
//     what the callers are after (genes_count.hip: BAM order inside a gene; pack_reads.hip: read order inside a tile bin).
// At the end: midas_snps_scan_u32 and midas_snps_sort_pairs, the two launches on host arrays (tests/test_gpu_sort.py).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <vector>

#include "ctx_internal.h"
#include "kernels.h"

namespace midas {
namespace {

constexpr int kScanThreads = 1024, kScanBlock = 4 * kScanThreads;      // counters per workgroup

// inclusive scan of one value per thread over a 1024-thread workgroup; returns the exclusive prefix of the thread and, in
// *total, the workgroup's sum
__device__ __forceinline__ uint32_t block_exclusive(uint32_t mine, uint32_t* wsum /* [16] */, uint32_t* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t inc = mine;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t o = __shfl_up(inc, d);
    if (lane >= d) inc += o;
  }
  if (lane == 63) wsum[wave] = inc;
  __syncthreads();
  uint32_t before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < 16; ++w) {
    const uint32_t x = wsum[w];
    before += w < wave ? x : 0u;
    all += x;
  }
  __syncthreads();       // (wsum may be written again by the caller's next round)
  *total = all;
  return before + inc - mine;
}

__global__ __launch_bounds__(kScanThreads) void scan_sums_kernel(const uint32_t* v, long long n, uint32_t* sums) {
  __shared__ uint32_t wsum[16];
  const long long i = (long long)blockIdx.x * kScanBlock + 4ll * threadIdx.x;
  uint32_t mine = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) mine += i + k < n ? v[i + k] : 0u;
  uint32_t total;
  (void)block_exclusive(mine, wsum, &total);
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// one workgroup: exclusive scan of m counters in place, 4096 at a time with a running carry
__global__ __launch_bounds__(kScanThreads) void scan_one_group_kernel(uint32_t* v, long long m) {
  __shared__ uint32_t wsum[16];
  uint32_t carry = 0;
  for (long long t0 = 0; t0 < m; t0 += kScanBlock) {
    const long long i = t0 + 4ll * threadIdx.x;
    uint32_t a[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) a[k] = i + k < m ? v[i + k] : 0u;
    uint32_t total;
    uint32_t run = carry + block_exclusive(a[0] + a[1] + a[2] + a[3], wsum, &total);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (i + k < m) v[i + k] = run;
      run += a[k];
    }
    carry += total;
  }
}

__global__ __launch_bounds__(kScanThreads) void scan_apply_kernel(const uint32_t* in, uint32_t* out, long long n, const uint32_t* sums) {
  __shared__ uint32_t wsum[16];
  const long long i = (long long)blockIdx.x * kScanBlock + 4ll * threadIdx.x;
  uint32_t a[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) a[k] = i + k < n ? in[i + k] : 0u;
  uint32_t total;
  uint32_t run = sums[blockIdx.x] + block_exclusive(a[0] + a[1] + a[2] + a[3], wsum, &total);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (i + k < n) out[i + k] = run;
    run += a[k];
  }
}

// ---- the sort --------------------------------------------------------------------------------------------------------------
// A workgroup owns kSortBlock consecutive pairs, each of its four waves a quarter of them, taken 64 at a time: the order of
// equal digits is (workgroup, wave, round, lane) = the input order.
//   hist     per workgroup the number of keys of every digit            -> hist[digit][workgroup]
//   scan     exclusive scan over hist in that (digit-major) order       -> where a workgroup's keys of a digit go
//   scatter  a wave finds, per round, the lanes that share a lane's digit (eight ballots), ranks the lane among them and
//            moves its pair to the digit's cursor of the wave (LDS), which the lowest of those lanes then advances
constexpr int kSortThreads = 256, kSortWaves = kSortThreads / 64, kSortRounds = 16;
constexpr int kSortBlock = kSortThreads * kSortRounds;      // 4096 pairs

__global__ __launch_bounds__(kSortThreads) void sort_hist_kernel(const uint32_t* key, long long n, int shift, uint32_t* hist, uint32_t n_blocks) {
  __shared__ uint32_t h[256];
  h[threadIdx.x] = 0u;
  __syncthreads();
  const long long base = (long long)blockIdx.x * kSortBlock;
#pragma unroll 4
  for (int r = 0; r < kSortRounds; ++r) {
    const long long i = base + (long long)r * kSortThreads + threadIdx.x;
    if (i < n) atomicAdd(&h[(key[i] >> shift) & 255u], 1u);
  }
  __syncthreads();
  hist[(size_t)threadIdx.x * n_blocks + blockIdx.x] = h[threadIdx.x];
}

template <class V>
__global__ __launch_bounds__(kSortThreads) void sort_scatter_kernel(const uint32_t* key, const V* val, long long n, int shift, const uint32_t* hist,
                                                                     uint32_t n_blocks, uint32_t* key_out, V* val_out) {
  __shared__ uint32_t cursor[kSortWaves][256];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int d = threadIdx.x; d < kSortWaves * 256; d += kSortThreads) (&cursor[0][0])[d] = 0u;
  __syncthreads();
  // the wave's own counts per digit ...
  const long long wbase = (long long)blockIdx.x * kSortBlock + (long long)wave * (kSortBlock / kSortWaves);
  for (int r = 0; r < kSortRounds; ++r) {
    const long long i = wbase + (long long)r * 64 + lane;
    if (i < n) atomicAdd(&cursor[wave][(key[i] >> shift) & 255u], 1u);
  }
  __syncthreads();
  // ... become where its keys of a digit start: the workgroup's place for the digit + the waves in front
  {
    const int d = threadIdx.x;       // 256 threads, 256 digits
    uint32_t at = hist[(size_t)d * n_blocks + blockIdx.x];
    for (int w = 0; w < kSortWaves; ++w) {
      const uint32_t c = cursor[w][d];
      cursor[w][d] = at;
      at += c;
    }
  }
  __syncthreads();
  const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
  for (int r = 0; r < kSortRounds; ++r) {
    const long long i = wbase + (long long)r * 64 + lane;
    const bool live = i < n;
    const uint32_t k = live ? key[i] : 0u;
    const uint32_t d = (k >> shift) & 255u;
    unsigned long long peers = __ballot(live);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const unsigned long long has = __ballot(live && ((d >> b) & 1u));
      peers &= ((d >> b) & 1u) ? has : ~has;
    }
    if (live) {
      const uint32_t at = cursor[wave][d] + (uint32_t)__popcll(peers & below);
      key_out[at] = k;
      val_out[at] = val[i];
    }
    // (LDS operations of one wave are carried out in order: every lane has read the cursor before its lowest peer moves it,
    // and the next round reads what this one wrote)
    if (live && (peers & below) == 0ull) cursor[wave][d] += (uint32_t)__popcll(peers);
  }
}

template <class V>
hipError_t sort_pairs(uint32_t* key_a, V* val_a, uint32_t* key_b, V* val_b, long long n, int bits, uint32_t* scratch, hipStream_t s,
                      uint32_t** key_sorted, V** val_sorted) {
  uint32_t* kin = key_a; V* vin = val_a; uint32_t* kout = key_b; V* vout = val_b;
  const uint32_t n_blocks = (uint32_t)((n + kSortBlock - 1) / kSortBlock);
  uint32_t* hist = scratch;
  uint32_t* sums = scratch + 256ull * n_blocks;
  for (int shift = 0; shift < bits && n > 0; shift += 8) {
    hipLaunchKernelGGL(sort_hist_kernel, dim3(n_blocks), dim3(kSortThreads), 0, s, kin, n, shift, hist, n_blocks);
    const hipError_t es = launch_scan_u32(hist, hist, 256ll * n_blocks, sums, s);
    if (es != hipSuccess) return es;
    hipLaunchKernelGGL(sort_scatter_kernel<V>, dim3(n_blocks), dim3(kSortThreads), 0, s, kin, vin, n, shift, hist, n_blocks, kout, vout);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    std::swap(kin, kout);
    std::swap(vin, vout);
  }
  *key_sorted = kin;
  *val_sorted = vin;
  return hipSuccess;
}

}  // namespace

size_t scan_scratch_words(long long n) { return (size_t)((n + kScanBlock - 1) / kScanBlock) + 1; }

hipError_t launch_scan_u32(const uint32_t* in, uint32_t* out, long long n, uint32_t* sums, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  const long long nb = (n + kScanBlock - 1) / kScanBlock;
  if (nb == 1 && in == out) {
    hipLaunchKernelGGL(scan_one_group_kernel, dim3(1), dim3(kScanThreads), 0, s, out, n);
    return hipGetLastError();
  }
  hipLaunchKernelGGL(scan_sums_kernel, dim3((unsigned)nb), dim3(kScanThreads), 0, s, in, n, sums);
  hipLaunchKernelGGL(scan_one_group_kernel, dim3(1), dim3(kScanThreads), 0, s, sums, nb);
  hipLaunchKernelGGL(scan_apply_kernel, dim3((unsigned)nb), dim3(kScanThreads), 0, s, in, out, n, sums);
  return hipGetLastError();
}

size_t sort_scratch_words(long long n) {
  const size_t nb = (size_t)((n > 0 ? n : 1) + kSortBlock - 1) / kSortBlock;
  return 256 * nb + scan_scratch_words(256ll * (long long)nb);
}

hipError_t launch_sort_pairs_u32(uint32_t* key_a, uint32_t* val_a, uint32_t* key_b, uint32_t* val_b, long long n, int bits, uint32_t* scratch,
                                 hipStream_t s, uint32_t** key_sorted, uint32_t** val_sorted) {
  return sort_pairs<uint32_t>(key_a, val_a, key_b, val_b, n, bits, scratch, s, key_sorted, val_sorted);
}

hipError_t launch_sort_pairs_f64(uint32_t* key_a, double* val_a, uint32_t* key_b, double* val_b, long long n, int bits, uint32_t* scratch,
                                 hipStream_t s, uint32_t** key_sorted, double** val_sorted) {
  return sort_pairs<double>(key_a, val_a, key_b, val_b, n, bits, scratch, s, key_sorted, val_sorted);
}

}  // namespace midas

// ---- test aids: the two primitives on host arrays, every device buffer between guard words ------------------------------------
namespace {
using midas_ctx::fail;

constexpr size_t kGuardWords = 64, kGuardBytes = kGuardWords * 4;
constexpr uint32_t kGuardWord = 0x5AC3A53Cu;

struct GuardPattern {
  uint32_t w[kGuardWords];
  GuardPattern() { std::fill(w, w + kGuardWords, kGuardWord); }
};
const GuardPattern kGuards;

// `bytes` of device memory (a multiple of 4) with kGuardWords words of kGuardWord right in front of it and right behind it.  What
// lies between starts out as 0xEE bytes: a word the launch fails to write must not look right because an earlier call's result
// lay in the same memory.
struct Guarded {
  midas_ctx::DeviceBuf buf;
  size_t bytes = 0;
  uint8_t* base() const { return static_cast<uint8_t*>(buf.p); }
  template <class T> T* data() const { return reinterpret_cast<T*>(base() + kGuardBytes); }
  hipError_t make(size_t n_bytes, hipStream_t s) {
    bytes = n_bytes;
    hipError_t e = hipMalloc(&buf.p, bytes + 2 * kGuardBytes);
    if (e == hipSuccess) e = hipMemsetAsync(buf.p, 0xEE, bytes + 2 * kGuardBytes, s);
    if (e == hipSuccess) e = hipMemcpyAsync(base(), kGuards.w, kGuardBytes, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(base() + kGuardBytes + bytes, kGuards.w, kGuardBytes, hipMemcpyHostToDevice, s);
    return e;
  }
  hipError_t put(const void* host, hipStream_t s) const {
    return bytes ? hipMemcpyAsync(base() + kGuardBytes, host, bytes, hipMemcpyHostToDevice, s) : hipSuccess;
  }
  // both guards down; *ok goes to false when a word of them differs (the stream is waited for)
  hipError_t check(hipStream_t s, bool* ok) const {
    uint32_t got[2 * kGuardWords];
    hipError_t e = hipMemcpyAsync(got, base(), kGuardBytes, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(got + kGuardWords, base() + kGuardBytes + bytes, kGuardBytes, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return e;
    for (size_t k = 0; k < 2 * kGuardWords; ++k)
      if (got[k] != kGuardWord) *ok = false;
    return hipSuccess;
  }
};

template <class V>
int32_t sort_pairs_guarded(midas_snps_ctx* ctx, int64_t n, int32_t bits, const uint32_t* key, const V* val, uint32_t* out_key, V* out_val,
                           int32_t* out_which, int32_t* out_guards_ok,
                           hipError_t (*launch)(uint32_t*, V*, uint32_t*, V*, long long, int, uint32_t*, hipStream_t, uint32_t**, V**)) {
  std::lock_guard<std::mutex> g(ctx->device_mutex);
  hipStream_t s = ctx->stream;
  Guarded key_a, key_b, val_a, val_b, scratch;
  HIP_TRY(ctx, key_a.make((size_t)n * 4, s));
  HIP_TRY(ctx, key_b.make((size_t)n * 4, s));
  HIP_TRY(ctx, val_a.make((size_t)n * sizeof(V), s));
  HIP_TRY(ctx, val_b.make((size_t)n * sizeof(V), s));
  HIP_TRY(ctx, scratch.make(midas::sort_scratch_words(n) * 4, s));
  HIP_TRY(ctx, key_a.put(key, s));
  HIP_TRY(ctx, val_a.put(val, s));
  uint32_t* key_sorted = nullptr;
  V* val_sorted = nullptr;
  HIP_TRY(ctx, launch(key_a.data<uint32_t>(), val_a.data<V>(), key_b.data<uint32_t>(), val_b.data<V>(), n, bits, scratch.data<uint32_t>(), s,
                      &key_sorted, &val_sorted));
  const bool in_a = key_sorted == key_a.data<uint32_t>() && val_sorted == val_a.data<V>();
  const bool in_b = key_sorted == key_b.data<uint32_t>() && val_sorted == val_b.data<V>();
  if (!in_a && !in_b) {
    (void)hipStreamSynchronize(s);
    return fail(ctx, MIDAS_SNPS_ERR_HIP, "sort_pairs: the launch named a result that is neither of the two buffer pairs");
  }
  if (n > 0) {
    HIP_TRY(ctx, hipMemcpyAsync(out_key, key_sorted, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipMemcpyAsync(out_val, val_sorted, (size_t)n * sizeof(V), hipMemcpyDeviceToHost, s));
  }
  bool ok = true;
  for (const Guarded* b : {&key_a, &key_b, &val_a, &val_b, &scratch}) HIP_TRY(ctx, b->check(s, &ok));
  *out_which = in_b ? 1 : 0;
  *out_guards_ok = ok ? 1 : 0;
  return MIDAS_SNPS_OK;
}
}  // namespace

extern "C" {

int32_t midas_snps_scan_u32(midas_snps_ctx* ctx, int64_t n, const uint32_t* in, int32_t in_place, uint32_t* out, int32_t* out_guards_ok,
                            int32_t* out_in_kept) {
  if (!ctx || n < 0 || (n > 0 && (!in || !out)) || !out_guards_ok || !out_in_kept) return MIDAS_SNPS_ERR_INVALID_ARG;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  std::lock_guard<std::mutex> g(ctx->device_mutex);
  hipStream_t s = ctx->stream;
  Guarded d_in, d_out, sums;
  HIP_TRY(ctx, d_in.make((size_t)n * 4, s));
  if (!in_place) HIP_TRY(ctx, d_out.make((size_t)n * 4, s));
  HIP_TRY(ctx, sums.make(midas::scan_scratch_words(n) * 4, s));
  HIP_TRY(ctx, d_in.put(in, s));
  uint32_t* const to = in_place ? d_in.data<uint32_t>() : d_out.data<uint32_t>();
  HIP_TRY(ctx, midas::launch_scan_u32(d_in.data<uint32_t>(), to, n, sums.data<uint32_t>(), s));
  if (n > 0) HIP_TRY(ctx, hipMemcpyAsync(out, to, (size_t)n * 4, hipMemcpyDeviceToHost, s));
  bool ok = true, kept = true;
  HIP_TRY(ctx, d_in.check(s, &ok));
  if (!in_place) HIP_TRY(ctx, d_out.check(s, &ok));
  HIP_TRY(ctx, sums.check(s, &ok));
  if (!in_place && n > 0) {
    std::vector<uint32_t> back((size_t)n);
    HIP_TRY(ctx, hipMemcpyAsync(back.data(), d_in.data<uint32_t>(), (size_t)n * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    kept = memcmp(back.data(), in, (size_t)n * 4) == 0;
  }
  *out_guards_ok = ok ? 1 : 0;
  *out_in_kept = kept ? 1 : 0;
  return MIDAS_SNPS_OK;
}

int32_t midas_snps_sort_pairs(midas_snps_ctx* ctx, int64_t n, int32_t bits, int32_t value_kind, const uint32_t* key, const void* val,
                              uint32_t* out_key, void* out_val, int32_t* out_which, int32_t* out_guards_ok) {
  if (!ctx || n < 0 || n > 0xFFFFFFFFll || bits < 0 || bits > 32 || (value_kind != 0 && value_kind != 1) ||
      (n > 0 && (!key || !val || !out_key || !out_val)) || !out_which || !out_guards_ok)
    return MIDAS_SNPS_ERR_INVALID_ARG;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (value_kind == 0)
    return sort_pairs_guarded<uint32_t>(ctx, n, bits, key, static_cast<const uint32_t*>(val), out_key, static_cast<uint32_t*>(out_val), out_which,
                                        out_guards_ok, midas::launch_sort_pairs_u32);
  return sort_pairs_guarded<double>(ctx, n, bits, key, static_cast<const double*>(val), out_key, static_cast<double*>(out_val), out_which,
                                    out_guards_ok, midas::launch_sort_pairs_f64);
}

}  // extern "C"
