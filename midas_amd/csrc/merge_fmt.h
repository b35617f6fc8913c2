// The cells of snps_freq.txt / snps_depth.txt as bytes, for the host and the device alike (merge_rows.hip; a stand-alone
// host program checks it against snprintf, tests/test_merge_rows_host.py).
//
// '{0:.3g}'.format(float(m) / d) without printf, for 0 < m <= d < 2^32.  printf rounds the decimal expansion of the DOUBLE
// x = fl(m / d) to three digits, half to even.  Here the three digits come from the RATIONAL m / d in integers:
//   k = the least k >= 0 with m 10^k >= d (so 10^-k <= m/d < 10^(1-k)); q, r = divmod(m 10^(k+2), d), q in [100, 1000).
//   2r != d: the rational is at least 1 / (2 d q) > 2^-43 of its value away from the three-digit boundary (q + 1/2) and the
//            double within 2^-53 of the rational: both round the same way.
//   2r == d: the rational IS the boundary; the double lies above it, below it or (when it is representable) on it -- found
//            exactly: x = M 2^E against (2q + 1) / (2 10^(k+2)), i.e. M 5^(k+2) against (2q + 1) 2^-(E+k+3), in 128 bits.
#pragma once
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MIDAS_FMT_HD __host__ __device__ inline
#else
#define MIDAS_FMT_HD inline
#endif

namespace midas_fmt {

// up to eight bytes of text, first byte lowest
struct Cell { uint64_t bytes; uint32_t len; };

MIDAS_FMT_HD void push(Cell& c, uint32_t ch) { c.bytes |= (uint64_t)ch << (8u * c.len); ++c.len; }

// decimal digits of v
MIDAS_FMT_HD uint32_t digits_u32(uint32_t v) {
  return v < 10u ? 1u : v < 100u ? 2u : v < 1000u ? 3u : v < 10000u ? 4u : v < 100000u ? 5u : v < 1000000u ? 6u
       : v < 10000000u ? 7u : v < 100000000u ? 8u : v < 1000000000u ? 9u : 10u;
}
MIDAS_FMT_HD uint32_t digits_u64(uint64_t v) {
  uint32_t n = 1;
  while (v >= 10ull) { v /= 10ull; ++n; }
  return n;
}

// -1 / 0 / +1: the double x (0 < x <= 1) below / on / above (2q + 1) / (2 10^(k+2))
MIDAS_FMT_HD int compare_with_boundary(double x, uint32_t q, uint32_t k) {
  uint64_t bits;
  memcpy(&bits, &x, 8);
  const int biased = (int)((bits >> 52) & 0x7FFu);
  const uint64_t M = biased ? ((bits & ((1ull << 52) - 1)) | (1ull << 52)) : (bits & ((1ull << 52) - 1));
  const int E = (biased ? biased : 1) - 1075;                  // x = M 2^E
  uint64_t p5 = 1;
  for (uint32_t i = 0; i < k + 2u; ++i) p5 *= 5ull;            // 5^(k+2) <= 5^12 < 2^28
  const unsigned __int128 lhs = (unsigned __int128)M * p5;     // < 2^81
  const int sh = -(E + (int)k + 3);                            // x <= 1 and M >= 2^52 (normal): E <= -52, sh >= 37
  if (sh < 0) return 1;
  if (sh >= 100) return -1;                                    // (2q + 1) 2^sh >= 2^107
  const unsigned __int128 rhs = (unsigned __int128)(2u * q + 1u) << sh;
  return lhs < rhs ? -1 : (lhs > rhs ? 1 : 0);
}

// '{0:.3g}'.format(float(m) / d) for 0 < m <= d; at most eight bytes
MIDAS_FMT_HD Cell format_freq(uint32_t m, uint32_t d) {
  uint64_t t = m;
  uint32_t k = 0;
  while (t < (uint64_t)d) { t *= 10ull; ++k; }                 // t = m 10^k in [d, 10 d): k <= 10
  const uint64_t num = t * 100ull;                             // < 1000 d < 2^42
  uint32_t q = (uint32_t)(num / d);
  const uint64_t r = num - (uint64_t)q * d;
  if (2ull * r > (uint64_t)d) {
    ++q;
  } else if (2ull * r == (uint64_t)d) {
    const int side = compare_with_boundary((double)m / (double)d, q, k);
    if (side > 0 || (side == 0 && (q & 1u))) ++q;
  }
  if (q == 1000u) { q = 100u; --k; }                           // (k >= 1 here: k == 0 means m == d, q == 100, r == 0)
  const uint32_t a = q / 100u, b = q / 10u % 10u, c = q % 10u;
  const uint32_t nd = c ? 3u : (b ? 2u : 1u);                  // %g strips trailing zeros
  Cell o{0ull, 0u};
  if (k <= 4u) {                                               // exponent >= -4: fixed notation
    if (k == 0u) {
      push(o, '0' + a);
      if (nd > 1u) push(o, '.');
    } else {
      push(o, '0');
      push(o, '.');
      for (uint32_t z = 1; z < k; ++z) push(o, '0');
      push(o, '0' + a);
    }
    if (nd > 1u) push(o, '0' + b);
    if (nd > 2u) push(o, '0' + c);
  } else {                                                     // d[.dd]e-XX
    push(o, '0' + a);
    if (nd > 1u) { push(o, '.'); push(o, '0' + b); }
    if (nd > 2u) push(o, '0' + c);
    push(o, 'e');
    push(o, '-');
    push(o, '0' + k / 10u);
    push(o, '0' + k % 10u);
  }
  return o;
}

// the cell of snps_freq.txt: '0' for an uncovered site or no minor allele
MIDAS_FMT_HD Cell freq_cell(uint32_t m, uint32_t d) {
  if (m == 0u || d == 0u) return Cell{(uint64_t)'0', 1u};
  return format_freq(m, d);
}

// decimal v at p (digits_* bytes); returns the byte after it
template <class Byte>
MIDAS_FMT_HD Byte* put_decimal(Byte* p, uint64_t v, uint32_t n_digits) {
  for (uint32_t i = n_digits; i-- > 0u;) { p[i] = (Byte)('0' + (uint32_t)(v % 10ull)); v /= 10ull; }
  return p + n_digits;
}
template <class Byte>
MIDAS_FMT_HD Byte* put_decimal32(Byte* p, uint32_t v, uint32_t n_digits) {
  for (uint32_t i = n_digits; i-- > 0u;) { p[i] = (Byte)('0' + v % 10u); v /= 10u; }
  return p + n_digits;
}

}  // namespace midas_fmt
