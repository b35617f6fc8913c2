// The packed path's work plan, the part that is plain arithmetic: which tiles are cut into parts and which counts start from
// zero.  No device code: checked on the CPU by tests/cpp/work_plan_check.cpp.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <utility>
#include <vector>

namespace midas {

constexpr int64_t kMaxTileParts = 4096;

struct __attribute__((visibility("hidden"))) WorkPlan {
  std::vector<uint32_t> items;                            // [n_items][4] {tile, part, n_parts, 0}: whole tiles first, then the parts
  int64_t n_whole = 0;                                    // items [0, n_whole) are whole tiles
  std::vector<std::pair<size_t, size_t>> zero_ranges;     // (first site, sites) of the split tiles, ascending, adjacent ones merged
  int64_t n_items() const { return (int64_t)(items.size() / 4); }
  bool any_split() const { return n_items() > n_whole; }
};

// Work items of the pileup kernel from the reads every tile will see: one per tile; a tile with very many reads (a coverage
// hot spot) is cut into parts that different workgroups process concurrently and merge with atomics -- otherwise one
// workgroup would walk it alone while the rest of the chip idles.  Split is only what would otherwise leave the chip idle: a
// tile holding more than twice a workgroup's fair share of all reads (and at least 2048), cut into parts of about one fair
// share (at least 1024 reads).  tiles[t] gives a tile's site_base and len (layout.h Tile).
template <class TileT>
__attribute__((visibility("hidden"))) inline WorkPlan plan_work_items(const uint32_t* tile_reads, const TileT* tiles, size_t n_tiles, int n_cu, int workgroups_per_cu) {
  int64_t total_reads = 0;
  for (size_t t = 0; t < n_tiles; ++t) total_reads += tile_reads[t];
  const int64_t fair = total_reads / ((int64_t)workgroups_per_cu * n_cu) + 1;
  int64_t split_reads = std::max<int64_t>(2048, 2 * fair), part_reads = std::max<int64_t>(1024, fair);
#ifdef MIDAS_SNPS_SPLIT_READS   // developer variants only (tools/build_variant.sh)
  split_reads = MIDAS_SNPS_SPLIT_READS;
  part_reads = split_reads > 1 ? split_reads / 2 : 1;
#endif
  WorkPlan plan;
  plan.items.reserve(n_tiles * 4 + 64);
  auto add = [&](size_t tile, int64_t part, int64_t n_parts) { for (uint32_t w : {(uint32_t)tile, (uint32_t)part, (uint32_t)n_parts, 0u}) plan.items.push_back(w); };
  for (size_t t = 0; t < n_tiles; ++t)     // whole tiles first ...
    if ((int64_t)tile_reads[t] <= split_reads) add(t, 0, 1);
  plan.n_whole = plan.n_items();
  for (size_t t = 0; t < n_tiles; ++t) {     // ... then the parts of split tiles
    if ((int64_t)tile_reads[t] <= split_reads) continue;
    const int64_t np = std::min<int64_t>(((int64_t)tile_reads[t] + part_reads - 1) / part_reads, kMaxTileParts);
    for (int64_t j = 0; j < np; ++j) add(t, j, np);
    const size_t first = (size_t)tiles[t].site_base, cnt = (size_t)tiles[t].len;
    if (!plan.zero_ranges.empty() && plan.zero_ranges.back().first + plan.zero_ranges.back().second == first) plan.zero_ranges.back().second += cnt;
    else plan.zero_ranges.emplace_back(first, cnt);
  }
  return plan;
}

}  // namespace midas
