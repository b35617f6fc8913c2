// The table of species ids (midas_amd/csrc/species_table.h) without a device: reads the ids from stdin, one a line as hex digits
// (an empty line is the empty id), builds the table with species_table_build and prints "table <size>", then for every id in the
// order given "<hash as 16 hex digits> <slot>", the slot being where the id lies -- or the one line "twice" when the build
// refuses the list.  Every id is also looked up the way sm_lookup_kernel probes: from hash & mask on until its own entry, never
// across an empty slot.  Stand-alone; returns 0, or says what failed and returns 1.
#include "species_table.h"

#include <cstdio>
#include <iostream>
#include <string>

using namespace midas;

int main() {
  std::string names, line;
  std::vector<int64_t> off(1, 0);
  while (std::getline(std::cin, line)) {
    if (line.size() % 2) { printf("FAILED: an odd number of hex digits on line %zu\n", off.size()); return 1; }
    for (size_t k = 0; k < line.size(); k += 2) names.push_back((char)std::stoi(line.substr(k, 2), nullptr, 16));
    off.push_back((int64_t)names.size());
  }
  const int32_t R = (int32_t)off.size() - 1;
  names.push_back('\0');                                   // (never read: the ids' storage is not null when every id is empty)
  std::vector<int32_t> slot;
  if (!species_table_build(names.data(), off.data(), R, &slot)) { printf("twice\n"); return 0; }
  const uint32_t table = (uint32_t)slot.size();
  if (table < 16 || (table & (table - 1)) || table < 2u * (uint32_t)R + 2u || (table > 16 && table / 2 >= 2u * (uint32_t)R + 2u)) {
    printf("FAILED: %u slots for %d ids\n", table, R);
    return 1;
  }
  std::vector<int32_t> at_of((size_t)R, -1);
  int32_t used = 0;
  for (uint32_t k = 0; k < table; ++k) {
    if (slot[k] == 0) continue;
    ++used;
    if (slot[k] < 0 || slot[k] > R || at_of[(size_t)slot[k] - 1] >= 0) { printf("FAILED: slot %u holds %d\n", k, slot[k]); return 1; }
    at_of[(size_t)slot[k] - 1] = (int32_t)k;
  }
  if (used != R) { printf("FAILED: %d of %d ids have a slot\n", used, R); return 1; }
  printf("table %u\n", table);
  for (int32_t g = 0; g < R; ++g) {
    const unsigned long long h = sm_hash(names.data() + off[(size_t)g], (uint32_t)(off[(size_t)g + 1] - off[(size_t)g]));
    uint32_t at = (uint32_t)h & (table - 1);
    while (slot[at] != g + 1) {
      if (slot[at] == 0) { printf("FAILED: the probe of id %d meets the empty slot %u\n", g, at); return 1; }
      at = (at + 1) & (table - 1);
    }
    printf("%016llx %u\n", h, at);
  }
  return 0;
}
