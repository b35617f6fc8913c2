// The context of the C ABI: create and destroy, the setters, status and error texts, page-locked host memory, and the copies
// between host and device (the copy kernel, the pinned staging ring).  See include/midas_snps.h for the contract.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <thread>

#include "../../include/midas_snps.h"
#include "ctx_internal.h"
#include "hostio.h"
#include "workers.h"

using namespace midas_ctx;

// Page-locked host memory the device writes and host threads read: non-coherent (coarse-grained) allocations are ordinary
// cached memory to the CPU -- the device's writes are visible once the stream has been synchronised, which every user
// here does -- where the default, coherent kind is mapped uncached on these hosts: the row formatter read its input
// 20 x slower from it (68 ms for 16 gzip members).
#ifndef MIDAS_SNPS_HOST_ALLOC_FLAGS
#define MIDAS_SNPS_HOST_ALLOC_FLAGS hipHostMallocNonCoherent
#endif
const unsigned int midas_ctx::kHostAllocFlags = MIDAS_SNPS_HOST_ALLOC_FLAGS;

namespace {

// Device -> host copy into caller memory.  Pinned destinations (midas_snps_host_alloc, or anything the caller registered
// with HIP) take one DMA; pageable ones go through the context's pinned ring, 32 MiB at a time, the DMA of chunk k + 1
// running while host threads move chunk k out (HIP's own pageable path reaches ~12 GB/s here, this one ~3x that).
void parallel_copy(uint8_t* dst, const uint8_t* src, size_t n) {
  const unsigned hw = (unsigned)midas::cpu_budget();
  size_t nt = hw >= 32 ? 12 : (hw >= 8 ? 4 : 1);
  if (n < ((size_t)4 << 20)) nt = 1;
  if (nt == 1) { memcpy(dst, src, n); return; }
  const size_t per = ((n + nt - 1) / nt + 63) & ~(size_t)63;
  std::atomic<size_t> next{0};
  midas::Workers::run((int)nt, [&] {
    for (;;) {
      const size_t lo = next.fetch_add(1) * per, hi = lo + per < n ? lo + per : n;
      if (lo >= hi) return;
      memcpy(dst + lo, src + lo, hi - lo);
    }
  });
}

// Results into page-locked host memory by the shader cores: stores to the mapped host pointer cross the link as posted
// writes.  The runtime's own device-to-host copy goes through the SDMA engines, which moved 16 GB/s here (255 MB of
// counts in 16 ms) where this kernel is limited by the link.
typedef uint32_t copy_u32x4 __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(256) void copy_out_kernel(copy_u32x4* __restrict__ dst, const copy_u32x4* __restrict__ src, size_t n16) {
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += stride) __builtin_nontemporal_store(src[i], &dst[i]);
}

}  // namespace

hipError_t midas_ctx::launch_copy16(void* dst, const void* src, size_t n16, int grid_blocks, hipStream_t s) {
  hipLaunchKernelGGL(copy_out_kernel, dim3(grid_blocks), dim3(256), 0, s, static_cast<copy_u32x4*>(dst), static_cast<const copy_u32x4*>(src), n16);
  return hipGetLastError();
}

int32_t midas_ctx::copy_to_host(midas_snps_ctx* ctx, void* dst, const void* src, size_t bytes, hipStream_t on) {
  if (bytes == 0) return MIDAS_SNPS_OK;
  hipStream_t s = on ? on : ctx->stream;
  hipPointerAttribute_t at;
  const bool pinned = hipPointerGetAttributes(&at, dst) == hipSuccess && at.type == hipMemoryTypeHost;
  (void)hipGetLastError();   // (an unregistered pointer is reported as an error: that is the pageable case)
#ifndef MIDAS_SNPS_NO_COPY_KERNEL
  if (pinned && bytes >= ((size_t)1 << 20) && (reinterpret_cast<uintptr_t>(dst) & 15u) == 0 && (reinterpret_cast<uintptr_t>(src) & 15u) == 0) {
    void* mapped = nullptr;
    if (hipHostGetDevicePointer(&mapped, dst, 0) == hipSuccess && mapped) {
      const size_t n16 = bytes / 16, tail = bytes - n16 * 16;
      HIP_TRY(ctx, launch_copy16(mapped, src, n16, 2048, s));
      if (tail) HIP_TRY(ctx, hipMemcpyAsync(static_cast<uint8_t*>(dst) + n16 * 16, static_cast<const uint8_t*>(src) + n16 * 16, tail, hipMemcpyDeviceToHost, s));
      HIP_TRY(ctx, hipStreamSynchronize(s));
      return MIDAS_SNPS_OK;
    }
    (void)hipGetLastError();
  }
#endif
  if (pinned || bytes < ((size_t)1 << 20)) {
    HIP_TRY(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    return MIDAS_SNPS_OK;
  }
  constexpr size_t kChunk = midas_snps_ctx::kStageBytes;
  std::lock_guard<std::mutex> ring(ctx->copy_mutex);
  ctx->stage_join();
  for (int k = 0; k < midas_snps_ctx::kStageSlots; ++k) {
    if (!ctx->stage[k]) HIP_TRY(ctx, hipHostMalloc(&ctx->stage[k], kChunk, kHostAllocFlags));
    if (!ctx->stage_ev[k]) HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->stage_ev[k], hipEventDisableTiming));
  }
  const size_t n_chunks = (bytes + kChunk - 1) / kChunk;
  auto issue = [&](size_t k) -> hipError_t {
    const size_t off = k * kChunk, n = std::min(kChunk, bytes - off);
    hipError_t e = hipSuccess;
    void* mapped = nullptr;
#ifndef MIDAS_SNPS_NO_COPY_KERNEL
    if ((reinterpret_cast<uintptr_t>(src) & 15u) == 0 && hipHostGetDevicePointer(&mapped, ctx->stage[k & 1], 0) != hipSuccess) mapped = nullptr;
    (void)hipGetLastError();
#endif
    if (mapped && n >= 16) {
      const size_t n16 = n / 16, tail = n - n16 * 16;
      e = launch_copy16(mapped, static_cast<const uint8_t*>(src) + off, n16, 2048, s);
      if (e == hipSuccess && tail)
        e = hipMemcpyAsync(static_cast<uint8_t*>(ctx->stage[k & 1]) + n16 * 16, static_cast<const uint8_t*>(src) + off + n16 * 16, tail, hipMemcpyDeviceToHost, s);
    } else {
      e = hipMemcpyAsync(ctx->stage[k & 1], static_cast<const uint8_t*>(src) + off, n, hipMemcpyDeviceToHost, s);
    }
    if (e == hipSuccess) e = hipEventRecord(ctx->stage_ev[k & 1], s);
    return e;
  };
  HIP_TRY(ctx, issue(0));
  for (size_t k = 0; k < n_chunks; ++k) {
    if (k + 1 < n_chunks) HIP_TRY(ctx, issue(k + 1));      // slot (k + 1) & 1 was emptied in the previous round
    HIP_TRY(ctx, hipEventSynchronize(ctx->stage_ev[k & 1]));
    const size_t off = k * kChunk, n = std::min(kChunk, bytes - off);
    parallel_copy(static_cast<uint8_t*>(dst) + off, static_cast<const uint8_t*>(ctx->stage[k & 1]), n);
  }
  return MIDAS_SNPS_OK;
}

namespace {
// Host bytes that are NOT page-locked (a mapped file, a malloc'd buffer) to the device through the context's pinned ring:
// several threads copy a chunk into a slot while the slot before it crosses the link.  The runtime's own pageable path
// stages through one thread: 14 GB/s out of a file mapping where this reaches the threads' copy rate.
// n bytes of a file into dst (a slot of the pinned ring) by several threads: the page cache's bytes, without a page of the
// file mapped for them (hostio.h, register_file_mapping)
bool parallel_pread(uint8_t* dst, int fd, size_t file_off, size_t n) {
  const unsigned hw = (unsigned)midas::cpu_budget();
  size_t nt = hw >= 32 ? 12 : (hw >= 16 ? 8 : (hw >= 8 ? 4 : (hw >= 2 ? 2 : 1)));
  static const int forced = [] { const char* e = getenv("MIDAS_SNPS_UPLOAD_THREADS"); return e ? atoi(e) : 0; }();
  if (forced > 0) nt = (size_t)std::min(forced, 64);
  if (n < ((size_t)4 << 20)) nt = 1;
  const size_t per = ((n + nt - 1) / nt + 4095) & ~(size_t)4095;
  std::atomic<int> bad{0};
  auto piece = [&](size_t k) {
    size_t off = k * per;
    const size_t end = std::min(n, off + per);
    while (off < end) {
      const ssize_t got = pread(fd, dst + off, end - off, (off_t)(file_off + off));
      if (got <= 0) { bad = 1; return; }
      off += (size_t)got;
    }
  };
  if (nt == 1) { piece(0); return bad == 0; }
  std::atomic<size_t> next{0};
  midas::Workers::run((int)nt, [&] {
    for (;;) {
      const size_t k = next.fetch_add(1);
      if (k >= nt) return;
      piece(k);
    }
  });
  return bad == 0;
}

}  // namespace

int32_t midas_ctx::copy_to_device_staged(midas_snps_ctx* ctx, void* dst, const void* src, size_t bytes, hipStream_t s) {
  constexpr size_t kChunk = midas_snps_ctx::kStageBytes;
  int src_fd = -1;
  size_t src_off = 0;
  const bool from_file = midas::file_of_mapping(src, bytes, &src_fd, &src_off);      // (a mapped BAM: read with pread, not through the mapping)
  if (bytes < 2 * kChunk && !from_file) {
    HIP_TRY(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s));
    return MIDAS_SNPS_OK;
  }
  std::lock_guard<std::mutex> ring(ctx->copy_mutex);
  ctx->stage_join();
  for (int k = 0; k < midas_snps_ctx::kStageSlots; ++k) {
    if (!ctx->stage[k]) HIP_TRY(ctx, hipHostMalloc(&ctx->stage[k], kChunk, kHostAllocFlags));
    if (!ctx->stage_ev[k]) HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->stage_ev[k], hipEventDisableTiming));
  }
  const size_t n_chunks = (bytes + kChunk - 1) / kChunk;
  for (size_t k = 0; k < n_chunks; ++k) {
    const int slot = (int)(k % midas_snps_ctx::kStageSlots);
    if (k >= (size_t)midas_snps_ctx::kStageSlots) HIP_TRY(ctx, hipEventSynchronize(ctx->stage_ev[slot]));      // the slot's last chunk is over
    const size_t off = k * kChunk, n = std::min(kChunk, bytes - off);
    if (from_file) {
      if (!parallel_pread(static_cast<uint8_t*>(ctx->stage[slot]), src_fd, src_off + off, n)) return fail(ctx, MIDAS_SNPS_ERR_BAD_LAYOUT, "short read on the BAM file");
    } else {
      parallel_copy(static_cast<uint8_t*>(ctx->stage[slot]), static_cast<const uint8_t*>(src) + off, n);
    }
    HIP_TRY(ctx, hipMemcpyAsync(static_cast<uint8_t*>(dst) + off, ctx->stage[slot], n, hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipEventRecord(ctx->stage_ev[slot], s));
  }
  // (the ring is free again when the caller next waits for the stream; the D2H path waits on the same events before it reuses a slot)
  for (int k = 0; k < midas_snps_ctx::kStageSlots; ++k) HIP_TRY(ctx, hipEventSynchronize(ctx->stage_ev[k]));
  return MIDAS_SNPS_OK;
}

void midas_ctx::device_free(void* p) { (void)hipFree(p); }

const char* midas_ctx::read_err_name(int32_t st) {
  switch (st) {
    case MIDAS_SNPS_ERR_READ_NO_SEQ: return "record has no SEQ (reference: TypeError in keep_read)";
    case MIDAS_SNPS_ERR_READ_NO_NM: return "record has no NM tag (reference: KeyError 'NM' in keep_read)";
    case MIDAS_SNPS_ERR_READ_ZERO_ALIGN: return "aligned length is 0 (reference: ZeroDivisionError in keep_read)";
    case MIDAS_SNPS_ERR_READ_NO_QUAL: return "record has no QUAL (reference: TypeError in np.mean)";
    case MIDAS_SNPS_ERR_READ_CIGAR_OVERRUN: return "CIGAR consumes more query than SEQ holds (reference: IndexError)";
    case MIDAS_SNPS_ERR_READ_BAD_CIGAR_OP: return "bad CIGAR op";
    default: return "unknown";
  }
}

extern "C" {

int32_t midas_snps_abi_version(void) { return MIDAS_SNPS_ABI_VERSION; }

int32_t midas_snps_cpu_budget(void) { return (int32_t)midas::cpu_budget(); }

const char* midas_snps_status_string(int32_t st) {
  switch (st) {
    case MIDAS_SNPS_OK: return "ok";
    case MIDAS_SNPS_ERR_INVALID_ARG: return "invalid argument";
    case MIDAS_SNPS_ERR_NO_DEVICE: return "no usable gfx950 device";
    case MIDAS_SNPS_ERR_HIP: return "HIP runtime error";
    case MIDAS_SNPS_ERR_OUT_OF_MEMORY: return "out of device memory";
    case MIDAS_SNPS_ERR_UNSUPPORTED: return "unsupported input";
    case MIDAS_SNPS_ERR_BAD_LAYOUT: return "inconsistent input layout";
    default: return (st >= 1 && st <= 6) ? read_err_name(st) : "unknown status";
  }
}

int32_t midas_snps_create(int32_t device_ordinal, midas_snps_ctx** out_ctx) {
  if (!out_ctx) return MIDAS_SNPS_ERR_INVALID_ARG;
  *out_ctx = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
    (void)hipGetLastError();
    return MIDAS_SNPS_ERR_NO_DEVICE;
  }
  if (device_ordinal < 0 || device_ordinal >= n) return MIDAS_SNPS_ERR_INVALID_ARG;
  midas_snps_ctx* ctx = new (std::nothrow) midas_snps_ctx();
  if (!ctx) return MIDAS_SNPS_ERR_OUT_OF_MEMORY;
  ctx->device = device_ordinal;
  if (hipSetDevice(device_ordinal) != hipSuccess ||
      hipGetDeviceProperties(&ctx->prop, device_ordinal) != hipSuccess ||
      hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking) != hipSuccess) {
    (void)hipGetLastError();
    delete ctx;
    return MIDAS_SNPS_ERR_NO_DEVICE;
  }
  // The kernels are built for gfx950 only; anything else cannot run them.
  if (strncmp(ctx->prop.gcnArchName, "gfx950", 6) != 0) {
    (void)hipStreamDestroy(ctx->own_stream);
    delete ctx;
    return MIDAS_SNPS_ERR_NO_DEVICE;
  }
  ctx->stream = ctx->own_stream;
  const char* coder = getenv("MIDAS_SNPS_ROW_CODER");
  ctx->row_coder = (coder && strcmp(coder, "host") == 0) ? MIDAS_SNPS_ROWS_HOST : MIDAS_SNPS_ROWS_DEVICE;
  // the pinned staging ring, page-locked beside whatever the caller does next (ctx_internal.h: stage_thread)
  ctx->stage_thread = std::thread([ctx] {
    if (hipSetDevice(ctx->device) != hipSuccess) { (void)hipGetLastError(); return; }
    for (int k = 0; k < midas_snps_ctx::kStageSlots; ++k)
      if (hipHostMalloc(&ctx->stage[k], midas_snps_ctx::kStageBytes, kHostAllocFlags) != hipSuccess) { (void)hipGetLastError(); ctx->stage[k] = nullptr; }
  });
  *out_ctx = ctx;
  return MIDAS_SNPS_OK;
}

void midas_snps_destroy(midas_snps_ctx* ctx) {
  if (!ctx) return;
  ctx->stage_join();
  (void)hipSetDevice(ctx->device);
  if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
  if (ctx->copy_stream) (void)hipStreamDestroy(ctx->copy_stream);
  ctx->row_buffers.clear();
  if (ctx->arena) ctx->arena->close();
  for (int k = 0; k < midas_snps_ctx::kStageSlots; ++k) {
    if (ctx->stage[k]) (void)hipHostFree(ctx->stage[k]);
    if (ctx->stage_ev[k]) (void)hipEventDestroy(ctx->stage_ev[k]);
  }
  delete ctx;
}

void* midas_snps_host_alloc(int64_t bytes) {
  void* p = nullptr;
  if (bytes <= 0 || hipHostMalloc(&p, (size_t)bytes, kHostAllocFlags) != hipSuccess) {
    (void)hipGetLastError();
    return nullptr;
  }
  return p;
}

void midas_snps_host_free(void* p) {
  if (p) (void)hipHostFree(p);
}

// The text is copied out under the context's error lock into a buffer of the calling thread (valid until that thread asks again):
// the table writers of one context run on several host threads.
const char* midas_snps_last_error(const midas_snps_ctx* ctx) {
  if (!ctx) return "NULL context";
  static thread_local std::string text;
  text = const_cast<midas_snps_ctx*>(ctx)->error_text();
  return text.c_str();
}

int64_t midas_snps_last_error_read(const midas_snps_ctx* ctx) { return ctx ? ctx->err_read : -1; }

int32_t midas_snps_set_stream(midas_snps_ctx* ctx, void* hip_stream) {
  if (!ctx) return MIDAS_SNPS_ERR_INVALID_ARG;
  ctx->stream = hip_stream ? reinterpret_cast<hipStream_t>(hip_stream) : ctx->own_stream;
  return MIDAS_SNPS_OK;
}

// Device-to-device copy rate of THIS device, with the library's own copy kernel (16 bytes per lane, streaming stores): the
// practical HBM ceiling a roofline fraction can be held against (the guide's 6.29 TB/s figure comes from such a kernel).
int32_t midas_snps_copy_rate(midas_snps_ctx* ctx, int64_t bytes, int32_t reps, double* out_gbps) {
  if (!ctx || !out_gbps || bytes < (1 << 20) || reps < 1) return MIDAS_SNPS_ERR_INVALID_ARG;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t n16 = (size_t)bytes / 16;
  DeviceBuf src, dst;
  HIP_TRY(ctx, hipMalloc(&src.p, n16 * 16));
  if (hipMalloc(&dst.p, n16 * 16) != hipSuccess) return fail(ctx, MIDAS_SNPS_ERR_OUT_OF_MEMORY, "copy_rate: out of device memory");
  hipEvent_t e0 = nullptr, e1 = nullptr;
  hipStream_t s = ctx->stream;
  int32_t st = MIDAS_SNPS_OK;
  float ms = 0.f;
  const int grid = ctx->prop.multiProcessorCount * 16;
  if (hipMemsetAsync(src.p, 0x5A, n16 * 16, s) != hipSuccess || hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) st = MIDAS_SNPS_ERR_HIP;
  if (st == MIDAS_SNPS_OK) {
    for (int k = 0; k < 2; ++k) (void)launch_copy16(dst.p, src.p, n16, grid, s);
    (void)hipEventRecord(e0, s);
    for (int k = 0; k < reps; ++k) (void)launch_copy16(dst.p, src.p, n16, grid, s);
    (void)hipEventRecord(e1, s);
    if (hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess || ms <= 0.f) st = MIDAS_SNPS_ERR_HIP;
  }
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  if (st != MIDAS_SNPS_OK) { (void)hipGetLastError(); return fail(ctx, st, "copy_rate: HIP runtime error"); }
  *out_gbps = 2.0 * (double)(n16 * 16) * reps / ((double)ms * 1e-3) / 1e9;
  return MIDAS_SNPS_OK;
}

int32_t midas_snps_copy_from_device(midas_snps_ctx* ctx, void* dst, const void* src, int64_t bytes) {
  if (!ctx || bytes < 0 || (bytes > 0 && (!dst || !src))) return MIDAS_SNPS_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> g(ctx->device_mutex);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  return copy_to_host(ctx, dst, src, (size_t)bytes);
}

int32_t midas_snps_set_row_coder(midas_snps_ctx* ctx, int32_t coder) {
  if (!ctx || (coder != MIDAS_SNPS_ROWS_DEVICE && coder != MIDAS_SNPS_ROWS_HOST)) return MIDAS_SNPS_ERR_INVALID_ARG;
  ctx->row_coder = coder;
  return MIDAS_SNPS_OK;
}

int32_t midas_snps_set_pad_rule(midas_snps_ctx* ctx, int32_t rule) {
  if (!ctx || (rule != MIDAS_SNPS_PAD_SPEC && rule != MIDAS_SNPS_PAD_PYSAM)) return MIDAS_SNPS_ERR_INVALID_ARG;
  ctx->pad_rule = rule;
  return MIDAS_SNPS_OK;
}

int32_t midas_snps_set_default_path(midas_snps_ctx* ctx, int32_t path) {
  if (!ctx || (path != MIDAS_SNPS_PATH_AUTO && path != MIDAS_SNPS_PATH_DIRECT && path != MIDAS_SNPS_PATH_PACKED && path != MIDAS_SNPS_PATH_LONG))
    return MIDAS_SNPS_ERR_INVALID_ARG;
  ctx->default_path = path;
  return MIDAS_SNPS_OK;
}

int32_t midas_snps_device_info(const midas_snps_ctx* ctx, char* name256, int32_t* n_cu, int64_t* hbm_bytes) {
  if (!ctx) return MIDAS_SNPS_ERR_INVALID_ARG;
  if (name256) snprintf(name256, 256, "%s (%s)", ctx->prop.name, ctx->prop.gcnArchName);
  if (n_cu) *n_cu = ctx->prop.multiProcessorCount;
  if (hbm_bytes) *hbm_bytes = (int64_t)ctx->prop.totalGlobalMem;
  return MIDAS_SNPS_OK;
}

}  // extern "C"
