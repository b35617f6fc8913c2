// What the kernels that read alignment records where they lie in an inflated BAM stream share (bam_walk.hip: the walk and the
// columns; genes_count.hip: the genes facts): unaligned little-endian reads -- a record starts at any byte -- and the NM tag.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace midas {

typedef uint32_t u32_a1 __attribute__((aligned(1)));
typedef uint16_t u16_a1 __attribute__((aligned(1)));
__device__ __forceinline__ uint32_t rd32(const uint8_t* p) { return *reinterpret_cast<const u32_a1*>(p); }
__device__ __forceinline__ uint32_t rd16(const uint8_t* p) { return *reinterpret_cast<const u16_a1*>(p); }

// NM:i (any integer width) from the aux block, or -1 (bam_host.cpp find_nm)
__device__ inline int32_t find_nm(const uint8_t* a, const uint8_t* end) {
  while (a + 3 <= end) {
    const char t0 = (char)a[0], t1 = (char)a[1], ty = (char)a[2];
    a += 3;
    unsigned long long sz = 0;
    switch (ty) {
      case 'A': case 'c': case 'C': sz = 1; break;
      case 's': case 'S': sz = 2; break;
      case 'i': case 'I': case 'f': sz = 4; break;
      case 'Z': case 'H': {
        const uint8_t* z = a;
        while (z < end && *z) ++z;
        if (z >= end) return -1;
        sz = (unsigned long long)(z - a) + 1ull;
        break;
      }
      case 'B': {
        if (a + 5 > end) return -1;
        const char st = (char)a[0];
        const unsigned long long cnt = rd32(a + 1);
        const unsigned long long es = (st == 'c' || st == 'C') ? 1 : (st == 's' || st == 'S') ? 2 : 4;
        sz = 5ull + cnt * es;
        break;
      }
      default: return -1;
    }
    if (sz > (unsigned long long)(end - a)) return -1;
    if (t0 == 'N' && t1 == 'M') {
      switch (ty) {
        case 'c': return (int8_t)a[0];
        case 'C': return a[0];
        case 's': return (int16_t)rd16(a);
        case 'S': return (int32_t)rd16(a);
        case 'i': return (int32_t)rd32(a);
        case 'I': { const uint32_t v = rd32(a); return v > 0x7FFFFFFFu ? 0x7FFFFFFF : (int32_t)v; }
        default: return -1;
      }
    }
    a += sz;
  }
  return -1;
}

}  // namespace midas
