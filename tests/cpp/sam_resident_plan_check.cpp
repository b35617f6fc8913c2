// The host arithmetic of the resident SAM decode (midas_amd/csrc/sam_resident_plan.h) held to a record-by-record model: the direct
// layout's units total recovered from the low 32 bits a scan keeps, the side buffer's entries and bytes, and the 32 GiB border on
// both sides.  Stand-alone: prints "ok <checks>" and returns 0, or says what failed and returns 1.
#define __host__
#define __device__
#include "sam_resident_plan.h"

#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

using namespace midas;

static long long n_checks = 0;
#define CHECK(cond, ...)                                       \
  do {                                                         \
    ++n_checks;                                                \
    if (!(cond)) {                                             \
      printf("FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond); \
      printf(__VA_ARGS__);                                     \
      printf("\n");                                            \
      exit(1);                                                 \
    }                                                          \
  } while (0)

struct Rec { uint32_t l_seq, n_cigar, exceptional; };

// the model: every record by itself, in 64 bits -- the payload run [cigar 4 c][sum 4][a byte a base] rounded up to 8 bytes, the raw
// [seq ceil(l / 2)][qual l] of a flagged record rounded up to 8 bytes
struct Model { unsigned long long units = 0, qual = 0, cigar = 0, side_entries = 0, side_bytes = 0; };
static Model model_of(const std::vector<Rec>& t) {
  Model m;
  for (const Rec& r : t) {
    const unsigned long long run = 4ull * r.n_cigar + 4ull + r.l_seq;
    m.units += (run + 7ull) / 8ull;
    m.qual += r.l_seq;
    m.cigar += r.n_cigar;
    if (r.exceptional) {
      ++m.side_entries;
      const unsigned long long raw = (r.l_seq + 1ull) / 2ull + r.l_seq;
      m.side_bytes += (raw + 7ull) / 8ull * 8ull;
    }
  }
  return m;
}

// what the device does: 32-bit sums of the per-record values (the scans' last entries)
static void check_table(const std::vector<Rec>& t, const char* what) {
  const Model m = model_of(t);
  uint32_t units32 = 0, ent32 = 0, side32 = 0;
  for (const Rec& r : t) {
    units32 += direct_payload_units(r.l_seq, r.n_cigar);
    ent32 += sam_side_entries(r.exceptional);
    side32 += sam_side_units(r.l_seq, r.exceptional);
  }
  const SamUnitsRange range = sam_units_range((long long)t.size(), (long long)m.qual, (long long)m.cigar);
  CHECK(range.lo <= m.units && m.units <= range.hi, "%s: %llu outside [%llu, %llu]", what, m.units, range.lo, range.hi);
  const unsigned long long total = sam_units_total(range, units32);
  CHECK(total == m.units, "%s: total %llu, model %llu", what, total, m.units);
  CHECK(sam_payload_fits(total) == (m.units * 8ull <= 0xFFFFFFFFull * 8ull), "%s: fits at %llu units", what, total);
  if (m.side_bytes / 8ull <= 0xFFFFFFFFull) {
    const SamSideSize z = sam_side_size(ent32, side32);
    CHECK(z.cap_entries == m.side_entries && z.cap_bytes == m.side_bytes, "%s: side %u / %llu, model %llu / %llu", what, z.cap_entries, z.cap_bytes,
          m.side_entries, m.side_bytes);
    CHECK(z.alloc_bytes == 32ull + 16ull * m.side_entries + m.side_bytes && z.fits, "%s: side allocation %llu", what, z.alloc_bytes);
    CHECK(m.side_bytes / 8ull <= sam_side_units_bound((long long)t.size(), (long long)m.qual), "%s: side bound", what);
  }
}

int main() {
  std::mt19937 rng(20240611u);
  // random tables: short and long reads, few and many ops, any share of flagged records
  for (int round = 0; round < 400; ++round) {
    std::vector<Rec> t((size_t)(rng() % 300u));
    const uint32_t share = rng() % 5u;
    for (Rec& r : t) {
      const uint32_t kind = rng() % 8u;
      r.l_seq = kind == 0 ? 0u : (kind == 1 ? rng() % 10u : (kind == 2 ? 250u + rng() % 10u : (kind == 3 ? 65530u + rng() % 5000u : rng() % 400u)));
      r.n_cigar = rng() % 4u == 0 ? 0u : (rng() % 16u == 0 ? 65535u - rng() % 3u : rng() % 70u);
      r.exceptional = share == 0 ? 0u : (share == 4 ? 1u : (rng() % 4u < share ? 1u : 0u));
    }
    check_table(t, "random");
  }
  check_table({}, "empty");
  check_table({{0, 0, 0}}, "one empty record");
  check_table({{0, 0, 1}}, "one empty flagged record");
  // the 32 GiB border: reads of a gigabase each (a line's limit) bring the total to 2^32 - 1 units, to 2^32, and beyond -- the 32-bit sum
  // wraps, the total does not
  {
    const uint32_t big = (1u << 30) - 4u;        // 2^27 units exactly: 4 + l = 2^30
    CHECK(direct_payload_units(big, 0) == (1u << 27), "a 2^27-unit read");
    std::vector<Rec> t(31, Rec{big, 0, 0});
    t.push_back(Rec{big - 8u, 0, 0});            // 32 * 2^27 - 1 = 2^32 - 1 units: the last total the layout addresses
    Model m = model_of(t);
    CHECK(m.units == 0xFFFFFFFFull, "border table: %llu", m.units);
    check_table(t, "2^32 - 1 units");
    CHECK(sam_payload_fits(sam_units_total(sam_units_range(32, (long long)m.qual, 0), 0xFFFFFFFFu)), "2^32 - 1 fits");
    t.back().l_seq = big;                        // 2^32 units: the sum's low word is 0
    m = model_of(t);
    CHECK(m.units == (1ull << 32), "border table + 1: %llu", m.units);
    check_table(t, "2^32 units");
    const unsigned long long over = sam_units_total(sam_units_range(32, (long long)m.qual, 0), 0u);
    CHECK(over == (1ull << 32) && !sam_payload_fits(over), "2^32 units do not fit (%llu)", over);
    for (int k = 0; k < 40; ++k) t.push_back(Rec{big - (uint32_t)(rng() % 1000u), 65535u, 1u});      // well beyond, flagged
    check_table(t, "far beyond");
  }
  // low bits that no total of the range has: the scan was not over these records
  {
    const SamUnitsRange r = sam_units_range(10, 1000, 20);      // 8 * total in [1120, 1190]
    CHECK(r.lo == 140 && r.hi == 148, "range [%llu, %llu]", r.lo, r.hi);
    CHECK(sam_units_total(r, 139u) == kSamUnitsUnknown && sam_units_total(r, 149u) == kSamUnitsUnknown, "outside the range");
    CHECK(sam_units_total(r, 140u) == 140 && sam_units_total(r, 148u) == 148, "the range's ends");
  }
  // the widest range the decode takes (2 * 10^9 records) still names one value; one too wide names none
  {
    const SamUnitsRange r = sam_units_range(kSamMaxRecords, kSamMaxQualBytes - 1, kSamMaxCigarOps - 1);
    CHECK(r.hi - r.lo < (1ull << 32), "width %llu", r.hi - r.lo);
    CHECK(sam_units_total(r, (uint32_t)r.hi) == r.hi && sam_units_total(r, (uint32_t)r.lo) == r.lo, "the widest range's ends");
    CHECK(sam_side_units_bound(kSamMaxRecords, kSamMaxQualBytes - 1) <= 0xFFFFFFFFull, "the side units cannot wrap");
    const SamUnitsRange w = sam_units_range(5000000000ll, 0, 0);
    CHECK(sam_units_total(w, 0u) == kSamUnitsUnknown, "a range of 2^32 or more");
  }
  printf("ok %lld\n", n_checks);
  return 0;
}
