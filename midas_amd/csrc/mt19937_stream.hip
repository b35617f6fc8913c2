// numpy's legacy random stream on the device, for snp_diversity.py --rand_reads --replace_reads (sites_scan.hip): MT19937 from
// the interpreter's own state, word by word as np.random.randint consumes it.
//   stream   ONE workgroup owns the stream: the 624-word state lives in LDS, twice (the block in use and the one being made).  A
//            refill is three dependent phases with a barrier behind each: words 0-226 from the old block, 227-453 from old words
//            and the new 0-226, 454-623 likewise (623 takes new[0] and new[396]).  Each word is tempered by the thread that made
//            it and written out with its accept flag, (w & mask) <= bound, and the masked value beside it.  A launch starts at
//            the position it is given, mid-block or not, and leaves state and position in device memory for the next one.  No
//            jump-ahead polynomial: the stream is generated in sequence, as the reference generates it
//   scatter  the accepted values of a launch in stream order, behind those already there: the exclusive scan of the flags
//            (device_sort.hip) is their place; the word's index in the launch goes beside the value -- what the host needs to
//            say where the stream stands behind the last value used
// At the end: midas_snps_mt19937_stream, the generator on host arrays (tests/test_gpu_resample.py).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <mutex>
#include <vector>

#include "ctx_internal.h"
#include "kernels.h"

namespace midas {
namespace {

constexpr int kMtN = 624, kMtM = 397, kMtThreads = 256;

__device__ __forceinline__ uint32_t mt_twist(uint32_t u, uint32_t v) {
  const uint32_t y = (u & 0x80000000u) | (v & 0x7FFFFFFFu);
  return (y >> 1) ^ ((v & 1u) ? 0x9908B0DFu : 0u);
}

__device__ __forceinline__ uint32_t mt_temper(uint32_t y) {
  y ^= y >> 11;
  y ^= (y << 7) & 0x9D2C5680u;
  y ^= (y << 15) & 0xEFC60000u;
  y ^= y >> 18;
  return y;
}

struct MtOut {
  uint32_t* raw;       // [n] the tempered words (nullptr: not wanted)
  uint32_t* flag;      // [n] 1: accepted (nullptr: not wanted, and neither is masked)
  uint32_t* masked;    // [n] w & mask
  uint32_t mask, bound;
};

__device__ __forceinline__ void mt_emit(const MtOut& o, long long at, uint32_t key) {
  const uint32_t w = mt_temper(key);
  if (o.raw) o.raw[at] = w;
  if (o.flag) {
    const uint32_t v = w & o.mask;
    o.flag[at] = v <= o.bound ? 1u : 0u;
    o.masked[at] = v;
  }
}

// state: 624 key words and the position (0 .. 624; 624: the block is used up), as np.random.get_state() gives them
__global__ __launch_bounds__(kMtThreads) void mt_stream_kernel(uint32_t* state, long long n, MtOut o) {
  __shared__ uint32_t key[2][kMtN];
  const int t = threadIdx.x;
  for (int i = t; i < kMtN; i += kMtThreads) key[0][i] = state[i];
  int pos = (int)state[kMtN];
  __syncthreads();
  int cur = 0;
  long long done = 0;
  // what is left of the block the state came with
  if (pos < kMtN && n > 0) {
    const int take = (int)(n < (long long)(kMtN - pos) ? n : (long long)(kMtN - pos));
    for (int i = t; i < take; i += kMtThreads) mt_emit(o, i, key[0][pos + i]);
    pos += take;
    done = take;
  }
  while (done < n) {                              // (uniform: every thread sees the same done and n)
    const uint32_t* a = key[cur];
    uint32_t* b = key[cur ^ 1];
    const long long left = n - done;
    const int take = (int)(left < (long long)kMtN ? left : (long long)kMtN);
    if (t < 227) {
      const uint32_t w = a[t + kMtM] ^ mt_twist(a[t], a[t + 1]);
      b[t] = w;
      if (t < take) mt_emit(o, done + t, w);
    }
    __syncthreads();
    if (t < 227) {
      const int i = 227 + t;
      const uint32_t w = b[t] ^ mt_twist(a[i], a[i + 1]);
      b[i] = w;
      if (i < take) mt_emit(o, done + i, w);
    }
    __syncthreads();
    if (t < 170) {
      const int i = 454 + t;
      const uint32_t w = b[i - 227] ^ mt_twist(a[i], i == kMtN - 1 ? b[0] : a[i + 1]);
      b[i] = w;
      if (i < take) mt_emit(o, done + i, w);
    }
    __syncthreads();
    cur ^= 1;
    pos = take;
    done += take;
  }
  for (int i = t; i < kMtN; i += kMtThreads) state[i] = key[cur][i];
  if (t == 0) state[kMtN] = (uint32_t)pos;
}

__global__ __launch_bounds__(256) void mt_scatter_kernel(const uint32_t* flag, const uint32_t* place, const uint32_t* masked, long long n,
                                                         uint32_t* accepted, uint32_t* accepted_at) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n || !flag[i]) return;
  accepted[place[i]] = masked[i];
  accepted_at[place[i]] = (uint32_t)i;
}

}  // namespace

hipError_t launch_mt_stream(uint32_t* state625, long long n, uint32_t* raw, uint32_t* flag, uint32_t* masked, uint32_t mask, uint32_t bound,
                            hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(mt_stream_kernel, dim3(1), dim3(kMtThreads), 0, s, state625, n, MtOut{raw, flag, masked, mask, bound});
  return hipGetLastError();
}

hipError_t launch_mt_scatter(const uint32_t* flag, const uint32_t* place, const uint32_t* masked, long long n, uint32_t* accepted,
                             uint32_t* accepted_at, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(mt_scatter_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, flag, place, masked, n, accepted, accepted_at);
  return hipGetLastError();
}

}  // namespace midas

// ---- test aid: the generator on host arrays, launch by launch -------------------------------------------------------------------
extern "C" int32_t midas_snps_mt19937_stream(midas_snps_ctx* ctx, const uint32_t* key624, int32_t pos, int64_t n_words, int64_t per_launch,
                                             int64_t bound, uint32_t* out_raw, uint8_t* out_flag, uint32_t* out_masked,
                                             uint32_t* out_key624, int32_t* out_pos) {
  if (!ctx || !key624 || pos < 0 || pos > 624 || n_words < 0 || per_launch < 0 || bound < 0 || bound > 0xFFFFFFFFll || !out_key624 || !out_pos ||
      (n_words > 0 && !out_raw))
    return MIDAS_SNPS_ERR_INVALID_ARG;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  std::lock_guard<std::mutex> g(ctx->device_mutex);
  hipStream_t s = ctx->stream;
  uint32_t mask = (uint32_t)bound;
  mask |= mask >> 1; mask |= mask >> 2; mask |= mask >> 4; mask |= mask >> 8; mask |= mask >> 16;
  const size_t n = (size_t)n_words;
  midas_ctx::DeviceBuf d_state, d_raw, d_flag, d_masked;
  HIP_TRY(ctx, hipMalloc(&d_state.p, 625 * 4));
  HIP_TRY(ctx, hipMalloc(&d_raw.p, n * 4 + 16));
  HIP_TRY(ctx, hipMalloc(&d_flag.p, n * 4 + 16));
  HIP_TRY(ctx, hipMalloc(&d_masked.p, n * 4 + 16));
  uint32_t st[625];
  for (int i = 0; i < 624; ++i) st[i] = key624[i];
  st[624] = (uint32_t)pos;
  HIP_TRY(ctx, hipMemcpyAsync(d_state.p, st, sizeof st, hipMemcpyHostToDevice, s));
  const long long step = per_launch > 0 ? per_launch : (n_words > 0 ? n_words : 1);
  for (long long at = 0; at < n_words; at += step) {
    const long long m = std::min<long long>(step, n_words - at);
    HIP_TRY(ctx, midas::launch_mt_stream(static_cast<uint32_t*>(d_state.p), m, static_cast<uint32_t*>(d_raw.p) + at,
                                         static_cast<uint32_t*>(d_flag.p) + at, static_cast<uint32_t*>(d_masked.p) + at, mask, (uint32_t)bound, s));
  }
  std::vector<uint32_t> flag(n);
  if (n > 0) {
    HIP_TRY(ctx, hipMemcpyAsync(out_raw, d_raw.p, n * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipMemcpyAsync(flag.data(), d_flag.p, n * 4, hipMemcpyDeviceToHost, s));
    if (out_masked) HIP_TRY(ctx, hipMemcpyAsync(out_masked, d_masked.p, n * 4, hipMemcpyDeviceToHost, s));
  }
  HIP_TRY(ctx, hipMemcpyAsync(st, d_state.p, sizeof st, hipMemcpyDeviceToHost, s));
  HIP_TRY(ctx, hipStreamSynchronize(s));
  if (out_flag) for (size_t i = 0; i < n; ++i) out_flag[i] = (uint8_t)flag[i];
  for (int i = 0; i < 624; ++i) out_key624[i] = st[i];
  *out_pos = (int32_t)st[624];
  return MIDAS_SNPS_OK;
}
