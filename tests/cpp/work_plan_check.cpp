// The packed path's work plan (midas_amd/csrc/work_plan.h) held to what it promises: which tiles are split, how the items are
// ordered, and which counts are zeroed before a run.
// Stand-alone: prints "ok <checks>" and returns 0, or says what failed and returns 1.
#include "work_plan.h"

#include <cstdio>
#include <cstdlib>

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

struct TileSpan { long long site_base; int len; };

// tiles back to back (the last one of every third short, as at a contig's end) with the given reads; returns the widest split seen
static long long check_case(const char* name, const std::vector<uint32_t>& reads, int n_cu, int wgs_per_cu, size_t want_split, size_t want_ranges) {
  const size_t nt = reads.size();
  std::vector<TileSpan> tiles(nt);
  long long site = 0, total = 0;
  for (size_t t = 0; t < nt; ++t) {
    tiles[t] = TileSpan{site, t % 3 == 2 ? 1000 + (int)t : 2048};
    site += tiles[t].len;
    total += reads[t];
  }
  const WorkPlan plan = plan_work_items(reads.data(), tiles.data(), nt, n_cu, wgs_per_cu);
  const WorkPlan again = plan_work_items(reads.data(), tiles.data(), nt, n_cu, wgs_per_cu);
  CHECK(plan.items == again.items && plan.n_whole == again.n_whole && plan.zero_ranges == again.zero_ranges, "%s: the same input gave another plan", name);
  CHECK(plan.items.size() % 4 == 0, "%s: %zu words", name, plan.items.size());
  // the rule, worked out here: a tile is split exactly when its reads exceed max(2048, 2 * fair)
  const long long fair = total / ((long long)wgs_per_cu * n_cu) + 1, split_above = std::max<long long>(2048, 2 * fair);
  std::vector<long long> np_of(nt, 0), parts_seen(nt, 0);
  long long max_np = 0;
  size_t n_split = 0;
  for (long long k = 0; k < plan.n_items(); ++k) {
    const uint32_t* it = &plan.items[(size_t)k * 4];
    const size_t t = it[0];
    CHECK(t < nt && it[3] == 0u && it[2] >= 1u, "%s: item %lld = {%u, %u, %u, %u}", name, k, it[0], it[1], it[2], it[3]);
    CHECK((k < plan.n_whole) == (it[2] == 1u), "%s: item %lld has %u parts, n_whole is %lld", name, k, it[2], (long long)plan.n_whole);
    if (np_of[t] == 0) np_of[t] = it[2];
    CHECK(np_of[t] == (long long)it[2], "%s: tile %zu with %lld and %u parts", name, t, np_of[t], it[2]);
    CHECK(it[1] == (uint32_t)parts_seen[t], "%s: tile %zu: part %u follows %lld parts", name, t, it[1], parts_seen[t]);      // parts 0..np-1, once each, in order
    parts_seen[t] += 1;
  }
  std::vector<std::pair<size_t, size_t>> want_zero;
  for (size_t t = 0; t < nt; ++t) {
    CHECK(parts_seen[t] == np_of[t] && np_of[t] >= 1, "%s: tile %zu appears %lld times of %lld", name, t, parts_seen[t], np_of[t]);
    const bool split = np_of[t] > 1;
    CHECK(split == ((long long)reads[t] > split_above), "%s: tile %zu with %u reads, split above %lld, has %lld parts", name, t, reads[t], split_above, np_of[t]);
    CHECK(np_of[t] <= 4096, "%s: tile %zu in %lld parts", name, t, np_of[t]);
    max_np = std::max(max_np, np_of[t]);
    if (!split) continue;
    ++n_split;
    if (!want_zero.empty() && want_zero.back().first + want_zero.back().second == (size_t)tiles[t].site_base) want_zero.back().second += (size_t)tiles[t].len;
    else want_zero.emplace_back((size_t)tiles[t].site_base, (size_t)tiles[t].len);
  }
  CHECK(n_split == want_split && plan.zero_ranges.size() == want_ranges, "%s: %zu tiles split, %zu zero ranges: the case was built for %zu and %zu", name, n_split,
        plan.zero_ranges.size(), want_split, want_ranges);
  // disjoint, ascending, merged where adjacent, and exactly the split tiles' sites
  for (size_t k = 1; k < plan.zero_ranges.size(); ++k)
    CHECK(plan.zero_ranges[k - 1].first + plan.zero_ranges[k - 1].second < plan.zero_ranges[k].first, "%s: zero ranges %zu and %zu touch or overlap", name, k - 1, k);
  CHECK(plan.zero_ranges == want_zero, "%s: %zu zero ranges, the split tiles make %zu", name, plan.zero_ranges.size(), want_zero.size());
  return max_np;
}

int main() {
  check_case("no tiles", {}, 256, 4, 0, 0);
  check_case("one tile", {100}, 256, 4, 0, 0);
  check_case("one hot tile alone", {3000000}, 256, 4, 1, 1);
  check_case("equal tiles", std::vector<uint32_t>(2000, 5000), 256, 4, 0, 0);
  check_case("one hot tile among five", {900, 1100, 400000, 1000, 950}, 256, 4, 1, 1);
  check_case("two hot tiles apart", {300000, 900, 350000, 1000}, 256, 4, 2, 2);
  const long long two = check_case("two adjacent hot tiles", {900, 300000, 350000, 1000, 950, 1200}, 256, 4, 2, 1);
  CHECK(two > 1, "two adjacent hot tiles: %lld parts at most", two);
  // 5 000 000 reads in one tile and enough workgroups that a fair share lies below the parts' floor of 1024 reads: 4883 parts
  // of 1024 would pass the limit of 4096
  CHECK((5000000 + 1023) / 1024 == 4883, "the case's arithmetic");
  const long long most = check_case("a tile beyond 4096 parts", {1000, 5000000, 1200}, 2048, 4, 1, 1);
  CHECK(most == 4096, "a tile beyond 4096 parts: %lld parts", most);
  printf("ok %lld\n", n_checks);
  return 0;
}
