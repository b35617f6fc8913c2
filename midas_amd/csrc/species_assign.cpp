// run_species.py, the serial part: reads whose best hits tie are given to one of the tied species, one read after another, each
// draw weighted by the reads every species holds by then (midas/run/species.py:104-119 -- the lists the reference counts are
// shared with the running totals, so a read assigned here changes the weights of the next).  Every step depends on the one
// before and is a few dozen instructions over a CSR of a few bytes a read: this runs on one host core on purpose.
//
// The two draws are the interpreter's: random.sample(ids, 1) when no tied species holds a read yet (an index below k from
// getrandbits(k.bit_length()), redrawn until it is), else numpy's legacy choice(ids, 1, p) (cumulative sums of p, divided by
// their last, one 53-bit double, the count of entries <= it).  Both generators are MT19937; their states come from the caller.
#include <cstdint>
#include <vector>

#include "../../include/midas_snps.h"

namespace midas {
namespace {

struct Mt19937 {
  uint32_t mt[624];
  int pos;
  uint32_t next() {
    if (pos >= 624) {
      for (int k = 0; k < 624; ++k) {
        const uint32_t y = (mt[k] & 0x80000000u) | (mt[(k + 1) % 624] & 0x7FFFFFFFu);
        mt[k] = mt[(k + 397) % 624] ^ (y >> 1) ^ ((y & 1u) ? 0x9908B0DFu : 0u);
      }
      pos = 0;
    }
    uint32_t y = mt[pos++];
    y ^= y >> 11;
    y ^= (y << 7) & 0x9D2C5680u;
    y ^= (y << 15) & 0xEFC60000u;
    y ^= y >> 18;
    return y;
  }
};

int bit_length(uint32_t k) {
  int b = 0;
  while (k) { ++b; k >>= 1; }
  return b;
}

}  // namespace
}  // namespace midas

extern "C" int32_t midas_species_assign(int64_t n_queries, const int64_t* indptr, const int32_t* hit_species, const int32_t* hit_aln,
                                        int32_t n_species, const uint32_t* py_state624, int32_t py_pos, const uint32_t* np_state624,
                                        int32_t np_pos, int64_t* inout_reads, int64_t* inout_aln, int64_t* out_draws2) {
  using namespace midas;
  if (n_queries < 0 || n_species < 0 || !py_state624 || !np_state624 || py_pos < 0 || py_pos > 624 || np_pos < 0 || np_pos > 624 ||
      (n_queries > 0 && (!indptr || !hit_species || !hit_aln || !inout_reads || !inout_aln)))
    return MIDAS_SNPS_ERR_INVALID_ARG;
  Mt19937 py, np;
  for (int k = 0; k < 624; ++k) { py.mt[k] = py_state624[k]; np.mt[k] = np_state624[k]; }
  py.pos = py_pos;
  np.pos = np_pos;
  int64_t draws_py = 0, draws_np = 0;
  std::vector<double> cdf;
  for (int64_t q = 0; q < n_queries; ++q) {
    const int64_t b = indptr[q], e = indptr[q + 1];
    if (e - b < 2 || e - b > 0x7FFFFFFF) return MIDAS_SNPS_ERR_BAD_LAYOUT;
    const uint32_t k = (uint32_t)(e - b);
    int64_t total = 0;
    for (int64_t h = b; h < e; ++h) {
      if (hit_species[h] < 0 || hit_species[h] >= n_species) return MIDAS_SNPS_ERR_BAD_LAYOUT;
      total += inout_reads[hit_species[h]];
    }
    uint32_t pick;
    if (total == 0) {
      const int bits = bit_length(k);
      do { pick = py.next() >> (32 - bits); ++draws_py; } while (pick >= k);
    } else {
      cdf.resize(k);
      double run = 0.0;
      for (uint32_t i = 0; i < k; ++i) {
        run += (double)inout_reads[hit_species[b + i]] / (double)total;
        cdf[i] = run;
      }
      const double last = cdf[k - 1];
      const uint32_t a = np.next() >> 5, c = np.next() >> 6;
      ++draws_np;
      const double u = ((double)a * 67108864.0 + (double)c) / 9007199254740992.0;
      pick = 0;
      for (uint32_t i = 0; i < k; ++i) pick += (cdf[i] / last <= u) ? 1u : 0u;
      if (pick >= k) return MIDAS_SNPS_ERR_BAD_LAYOUT;      // (numpy: an index past the list; cannot happen while u < 1 = cdf[k-1]/last)
    }
    const int32_t sp = hit_species[b + pick];
    int64_t first = b;                                      // the read carries the aln of the first hit of the drawn species
    while (hit_species[first] != sp) ++first;
    inout_reads[sp] += 1;
    inout_aln[sp] += hit_aln[first];
  }
  if (out_draws2) { out_draws2[0] = draws_py; out_draws2[1] = draws_np; }
  return MIDAS_SNPS_OK;
}
