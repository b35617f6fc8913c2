// The open-addressing table of species_info.txt's ids that merge_species.py looks every profile line up in (species_merge.hip):
// the hash of an id's bytes and the host loop that fills the slots.  The size is 16, doubled while it is below 2 R + 2, so the
// table is at most half full and an empty slot ends every probe; slot = species + 1, 0 = empty; an id goes into the first empty
// slot from hash & (size - 1) on, in the order of the list.  Host and device compile the same lines; a host compiler takes this
// file alone (tests/cpp/species_table_check.cpp).
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

#if defined(__HIPCC__)
#define MIDAS_ST_HD __host__ __device__
#else
#define MIDAS_ST_HD
#endif

namespace midas {

MIDAS_ST_HD inline unsigned long long sm_hash(const char* s, uint32_t n) {   // FNV-1a, then MurmurHash3's finaliser
  unsigned long long h = 0xCBF29CE484222325ull;
  for (uint32_t k = 0; k < n; ++k) { h ^= (unsigned char)s[k]; h *= 0x100000001B3ull; }
  h ^= h >> 33; h *= 0xFF51AFD7ED558CCDull; h ^= h >> 33; h *= 0xC4CEB9FE1A85EC53ull; h ^= h >> 33;
  return h;
}

// slot[] over the R ids, id g = ids[off[g], off[g + 1]) -> true, or false when an id is listed twice
inline bool species_table_build(const char* ids, const int64_t* off, int32_t R, std::vector<int32_t>* slot_out) {
  uint32_t table = 16;
  while (table < 2u * (uint32_t)R + 2u) table <<= 1;
  std::vector<int32_t> slot(table, 0);
  for (int32_t g = 0; g < R; ++g) {
    const char* nm = ids + off[g];
    const uint32_t len = (uint32_t)(off[g + 1] - off[g]);
    uint32_t at = (uint32_t)sm_hash(nm, len) & (table - 1);
    while (slot[at]) {
      const int32_t o = slot[at] - 1;
      if ((uint32_t)(off[o + 1] - off[o]) == len && std::memcmp(ids + off[o], nm, len) == 0) return false;
      at = (at + 1) & (table - 1);
    }
    slot[at] = g + 1;
  }
  slot_out->swap(slot);
  return true;
}

}  // namespace midas
