// The direct layout's base bytes (layout.h dense_byte) written and read back by groups of adjacent lanes of one wavefront:
// the producers (index_direct.hip direct_layout_fill_kernel, bam_walk.hip bam_direct_kernel) encode a read's 4-bit SEQ + QUAL,
// the raw-column cut (bgzf_inflate.hip bam_payload_kernel) decodes them and then applies the side buffer's exact copies.
// (Host code may include it with its own stand-ins for the few HIP names it uses: tests/test_dense_layout_host.py runs encode /
// decode with G = 1 against layout.h's definitions.)
#pragma once
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#endif
#include "layout.h"

namespace midas {
namespace dense {

typedef uint32_t u32_ua __attribute__((aligned(1)));
typedef unsigned long long u64_ua __attribute__((aligned(1)));

// a 64-bit value broadcast from lane `src` of the wavefront
__device__ __forceinline__ unsigned long long shfl64(unsigned long long v, int src) {
  const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src), hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), src);
  return ((unsigned long long)hi << 32) | lo;
}

// One base, branch-free: the A/C/G/T code of each 4-bit SEQ code from one table (4 bits a code: 0-3 A/C/G/T, 8 anything else,
// 9 N) -- what layout.h dense_byte / dense_exact say, with fewer instructions a base (the producers run it on every base).
constexpr unsigned long long kNibClass = 0x9888888388828108ull;
struct Base { uint32_t byte, exact, clamp; };
__device__ __forceinline__ Base base_of(uint32_t nib, uint32_t q) {
  const uint32_t t = (uint32_t)(kNibClass >> (4u * nib)) & 15u;
  const bool acgt = t < 4u;
  Base b;
  b.byte = acgt ? (((q < kDenseMaxQual ? q : kDenseMaxQual) + 13u) << 2) | t : (q < kDenseMaxOtherQual ? q : kDenseMaxOtherQual);
  b.exact = acgt ? (q <= kDenseMaxQual ? 1u : 0u) : ((t == 9u && q <= kDenseMaxOtherQual) ? 1u : 0u);
  b.clamp = (acgt && q > kDenseMaxQual) ? 1u : 0u;
  return b;
}

// One read: its sum word at dst (4-byte aligned) and its l base bytes behind it, the rest of its last 8-byte unit zeroed (dst +
// 4 + l .. dst + room), by the G lanes gl = 0 .. G - 1 of a group (adjacent lanes, the group aligned to G in the wavefront).
// seq: ceil(l / 2) bytes of 4-bit codes, qual: l bytes, any alignment; eight bases a lane and step.  Returns on every lane of
// the group whether the read is exceptional (layout.h dense_exact, the pad nibble); raises kDenseClampedQual in side->flags.
template <int G>
__device__ __forceinline__ bool encode(uint8_t* dst, uint32_t room, const uint8_t* seq, const uint8_t* qual, uint32_t l, int gl, DenseSide* side) {
  uint32_t sum = 0u, exc = 0u, clamp = 0u;
  for (uint32_t k = (uint32_t)gl * 8u; k < l; k += 8u * G) {
    const uint32_t n = l - k < 8u ? l - k : 8u;
    uint32_t s;
    unsigned long long qa;
    if (n == 8u) {
      s = *reinterpret_cast<const u32_ua*>(seq + (k >> 1));
      qa = *reinterpret_cast<const u64_ua*>(qual + k);
    } else {
      s = 0u; qa = 0ull;
      for (uint32_t j = 0; j < (n + 1u) >> 1; ++j) s |= (uint32_t)seq[(k >> 1) + j] << (8u * j);
      for (uint32_t j = 0; j < n; ++j) qa |= (unsigned long long)qual[k + j] << (8u * j);
      if ((l & 1u) && (s >> (8u * ((n - 1u) >> 1)) & 15u) != 0u) exc = 1u;     // (odd l: the last byte's low nibble is padding)
    }
    unsigned long long out = 0ull;
    for (uint32_t j = 0; j < n; ++j) {
      const uint32_t nib = (s >> (8u * (j >> 1) + ((j & 1u) ? 0u : 4u))) & 15u;
      const uint32_t q = (uint32_t)(qa >> (8u * j)) & 0xFFu;
      const Base b = base_of(nib, q);
      out |= (unsigned long long)b.byte << (8u * j);
      sum += q;
      exc |= b.exact ^ 1u;
      clamp |= b.clamp;
    }
    if (n == 8u) *reinterpret_cast<u64_ua*>(dst + 4u + k) = out;
    else for (uint32_t j = 0; j < n; ++j) dst[4u + k + j] = (uint8_t)(out >> (8u * j));
  }
  // (the two flags of the group by one ballot each, the sum by log2(G) exchanges)
  const int lane = (int)(threadIdx.x & 63u);
  const unsigned long long gmask = (G >= 64 ? ~0ull : ((1ull << G) - 1ull)) << ((lane - gl) & 63);
  exc = (__ballot(exc != 0u) & gmask) != 0ull ? 1u : 0u;
  clamp = (__ballot(clamp != 0u) & gmask) != 0ull ? 1u : 0u;
  for (int d = G / 2; d >= 1; d >>= 1) sum += (uint32_t)__shfl_xor((int)sum, d);
  if (gl == 0) {
    const uint32_t absent = (l > 0u && qual[0] == 0xFFu) ? kDenseQualAbsent : 0u;
    *reinterpret_cast<uint32_t*>(dst) = sum | absent;
    for (uint32_t j = 4u + l; j < room; ++j) dst[j] = 0;
    if (clamp) atomicOr(&side->flags, kDenseClampedQual);
  }
  return exc != 0u;
}

// An exceptional read's raw [seq][qual] into the side buffer (layout.h DenseSide), by the G lanes of its group (every lane of
// the group calls it).  No room: kDenseSideOverflow, nothing stored.
template <int G>
__device__ __forceinline__ void side_copy(DenseSide* side, unsigned long long read, const uint8_t* seq, const uint8_t* qual, uint32_t l, int gl) {
  const int lane = (int)(threadIdx.x & 63u);
  unsigned long long off = ~0ull;
  if (gl == 0) {
    const unsigned long long room = dense_side_room(l);
    const unsigned long long r = atomicAdd(&side->bump, (1ull << kDenseSideEntryShift) | (room >> 3));
    const unsigned long long e = r >> kDenseSideEntryShift, o = (r & kDenseSideMaxField) << 3;
    if (e < side->cap_entries && o + room <= side->cap_bytes) {
      DenseSideEntry ent;
      ent.read = read; ent.off = o;
      dense_side_entries(side)[e] = ent;
      off = o;
    } else {
      atomicOr(&side->flags, kDenseSideOverflow);
    }
  }
  off = shfl64(off, lane - gl);
  if (off == ~0ull) return;
  uint8_t* d = dense_side_data(side) + off;
  const uint32_t ns = (l + 1u) >> 1;
  for (uint32_t j = (uint32_t)gl; j < ns; j += G) d[j] = seq[j];
  for (uint32_t j = (uint32_t)gl; j < l; j += G) d[ns + j] = qual[j];
}

// The l base bytes at src back to 4-bit SEQ (the pad nibble zero) and QUAL, by the G lanes of a group: exact for a read that is
// not exceptional (an exceptional one is overwritten by the side buffer's copy behind this).
template <int G>
__device__ __forceinline__ void decode(uint8_t* seq, uint8_t* qual, const uint8_t* src, uint32_t l, int gl) {
  for (uint32_t k = (uint32_t)gl * 8u; k < l; k += 8u * G) {
    const uint32_t n = l - k < 8u ? l - k : 8u;
    unsigned long long b = 0ull;
    if (n == 8u) b = *reinterpret_cast<const u64_ua*>(src + k);
    else for (uint32_t j = 0; j < n; ++j) b |= (unsigned long long)src[k + j] << (8u * j);
    uint32_t s = 0u;
    unsigned long long q = 0ull;
    for (uint32_t j = 0; j < n; ++j) {
      const uint32_t x = (uint32_t)(b >> (8u * j)) & 0xFFu;
      s |= dense_nibble(x) << (8u * (j >> 1) + ((j & 1u) ? 0u : 4u));
      q |= (unsigned long long)dense_qual(x) << (8u * j);
    }
    if (n == 8u) {
      *reinterpret_cast<u32_ua*>(seq + (k >> 1)) = s;
      *reinterpret_cast<u64_ua*>(qual + k) = q;
    } else {
      for (uint32_t j = 0; j < (n + 1u) >> 1; ++j) seq[(k >> 1) + j] = (uint8_t)(s >> (8u * j));
      for (uint32_t j = 0; j < n; ++j) qual[k + j] = (uint8_t)(q >> (8u * j));
    }
  }
}

}  // namespace dense
}  // namespace midas
