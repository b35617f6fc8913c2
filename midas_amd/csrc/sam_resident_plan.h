// The host arithmetic of the resident SAM decode (sam_scan.hip, midas_sam_load_resident), free of any device call so that a plain
// C++ compiler builds it and tests/cpp/sam_resident_plan_check.cpp can hold it to a record-by-record model: what a record adds to
// the side buffer, the direct layout's units total recovered from a 32-bit scan, the side buffer's sizes, and the limits.
// (A plain compiler defines __host__ and __device__ away in front of it, as tests/test_dense_layout_host.py does for layout.h.)
#pragma once
#include <stdint.h>

#include "layout.h"

namespace midas {

// The decode's limits (include/midas_snps.h): the sorted offsets are 32-bit scans.
constexpr long long kSamMaxRecords = 2000000000ll;
constexpr long long kSamMaxQualBytes = 1ll << 32;       // (exclusive)
constexpr long long kSamMaxCigarOps = 1ll << 32;        // (exclusive)

// What a record reserves in the side buffer (layout.h DenseSide) when pass 2 flagged it exceptional: one entry and its raw
// [seq][qual] in 8-byte units.  The kernel that sizes the buffer and the model of the check both call these.
__host__ __device__ inline uint32_t sam_side_entries(uint32_t exceptional) { return exceptional ? 1u : 0u; }
__host__ __device__ inline uint32_t sam_side_units(uint32_t l_seq, uint32_t exceptional) {
  return exceptional ? (uint32_t)(dense_side_room(l_seq) >> 3) : 0u;
}

// The units of the whole payload lie in a range the column totals give: a record of l bases and c ops takes
// (4 c + 4 + l + 7) >> 3 units, so 8 * units lies in [4 c + 4 + l, 4 c + 4 + l + 7], and over n records of Q bases and C ops
// 8 * total lies in [S, S + 7 n] with S = 4 C + 4 n + Q.  The range is narrower than 2^32 for every n the decode takes
// (7 n / 8 < 2^31 for n <= 2 * 10^9), so the total's low 32 bits -- all a 32-bit scan keeps -- name one value in it.
struct SamUnitsRange { unsigned long long lo, hi; };
inline SamUnitsRange sam_units_range(long long n, long long qual_bytes, long long n_cigar) {
  const unsigned long long s = 4ull * (unsigned long long)n_cigar + 4ull * (unsigned long long)n + (unsigned long long)qual_bytes;
  return SamUnitsRange{(s + 7ull) >> 3, (s + 7ull * (unsigned long long)n) >> 3};
}
constexpr unsigned long long kSamUnitsUnknown = ~0ull;
// the total whose low 32 bits the scan's last entry holds; kSamUnitsUnknown: no value of the range has them (the scan's input was
// not these records'), or the range is too wide to name one
inline unsigned long long sam_units_total(const SamUnitsRange& r, uint32_t scanned_low32) {
  if (r.hi < r.lo || r.hi - r.lo >= (1ull << 32)) return kSamUnitsUnknown;
  const unsigned long long t = r.lo + (uint32_t)(scanned_low32 - (uint32_t)r.lo);
  return t <= r.hi ? t : kSamUnitsUnknown;
}
// DirectRec::off8 is 32 bits of 8-byte units: 32 GiB of payload
inline bool sam_payload_fits(unsigned long long units_total) { return units_total <= kMaxDirectPayloadUnits; }

// The side buffer, sized exactly in front of the launch from the two scans' totals.  Neither scan can wrap under the limits above:
// the entries are at most n, the units at most (1.5 Q + 7.5 n) / 8 < 2^32 (sam_side_units_bound).
inline unsigned long long sam_side_units_bound(long long n, long long qual_bytes) {
  return (3ull * (unsigned long long)qual_bytes + 15ull * (unsigned long long)n) / 16ull + 1ull;
}
struct SamSideSize {
  uint32_t cap_entries;
  unsigned long long cap_bytes;       // of data
  unsigned long long alloc_bytes;     // header + entries + data
  bool fits;                          // no reservation can carry out of a field of DenseSide::bump
};
inline SamSideSize sam_side_size(uint32_t entries_total, uint32_t units_total) {
  SamSideSize z;
  z.cap_entries = entries_total;
  z.cap_bytes = (unsigned long long)units_total << 3;
  z.alloc_bytes = dense_side_bytes(z.cap_entries, z.cap_bytes);
  z.fits = dense_side_fits(entries_total, units_total);
  return z;
}

}  // namespace midas
