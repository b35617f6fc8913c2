// The sizes of a walk by row groups (midas_amd/csrc/row_group_plan.h) held to the three formulas the function replaced, written
// out as they stood: RowGroups::init over two matrices, midas_genes_compare and midas_genes_linkage over one.  Random requests
// and sizes, and every border: zero and non-zero requests, a quarter of the free memory below 1 MiB, a text shorter than 64
// bytes, a row bound of 1 (and of 0), a chunk at 2^30.  Stand-alone: prints "ok <checks>" and returns 0, or says what failed and
// returns 1.
#include "row_group_plan.h"

#include <cstdio>
#include <cstdlib>
#include <random>

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

// RowGroups::init as it stood (sites_rows.h): the chunks of two matrices
static RowGroupPlan sites_formula(size_t free_b, long long G, long long chunk_bytes, long long freq_bytes, long long depth_bytes, long long n_sites_max,
                                  long long per_row) {
  constexpr long long kMax = (1ll << 30);
  if (G == 0 || chunk_bytes == 0) {
    const long long budget = (long long)(free_b / 4);
    if (chunk_bytes == 0) chunk_bytes = std::min<long long>(kMax, std::max<long long>(1 << 20, budget / 8));
    if (G == 0) G = std::max<long long>(1, (budget - std::min(budget / 2, 5 * chunk_bytes / 2)) / per_row);
  }
  chunk_bytes = std::min(std::max<long long>(chunk_bytes, 64), kMax);
  chunk_bytes = std::min(chunk_bytes, std::max<long long>(64, std::max(freq_bytes, depth_bytes) + 1));
  G = std::min<long long>(std::min<long long>(G, n_sites_max), chunk_bytes);
  G = std::max<long long>(G, 1);
  return RowGroupPlan{G, chunk_bytes};
}

// midas_genes_compare and midas_genes_linkage as they stood: the same lines in both, one matrix
static RowGroupPlan genes_formula(size_t free_b, long long G, long long chunk_bytes, long long text_bytes, long long n_rows_max, long long per_row) {
  constexpr long long kMax = 1ll << 30;
  if (G == 0 || chunk_bytes == 0) {
    const long long budget = (long long)(free_b / 4);
    if (chunk_bytes == 0) chunk_bytes = std::min<long long>(kMax, std::max<long long>(1 << 20, budget / 4));
    if (G == 0) G = std::max<long long>(1, (budget - std::min(budget / 2, 5 * chunk_bytes / 4)) / per_row);
  }
  chunk_bytes = std::min(std::max<long long>(chunk_bytes, 64), kMax);
  chunk_bytes = std::min(chunk_bytes, std::max<long long>(64, (long long)text_bytes + 1));
  G = std::max<long long>(1, std::min<long long>(std::min<long long>(G, n_rows_max), chunk_bytes));
  return RowGroupPlan{G, chunk_bytes};
}

static void check_one(size_t free_b, long long G, long long chunk, long long text, long long other, long long rows, long long per_row) {
  const RowGroupPlan g = plan_row_groups(free_b, G, chunk, 1, text, rows, per_row), wg = genes_formula(free_b, G, chunk, text, rows, per_row);
  CHECK(g.G == wg.G && g.chunk_bytes == wg.chunk_bytes, "one matrix: free %zu, asked %lld / %lld, text %lld, rows %lld, per row %lld: %lld / %lld, the formula has %lld / %lld",
        free_b, G, chunk, text, rows, per_row, g.G, g.chunk_bytes, wg.G, wg.chunk_bytes);
  const RowGroupPlan s = plan_row_groups(free_b, G, chunk, 2, std::max(text, other), rows, per_row), ws = sites_formula(free_b, G, chunk, text, other, rows, per_row);
  CHECK(s.G == ws.G && s.chunk_bytes == ws.chunk_bytes, "two matrices: free %zu, asked %lld / %lld, texts %lld and %lld, rows %lld, per row %lld: %lld / %lld, the formula has %lld / %lld",
        free_b, G, chunk, text, other, rows, per_row, s.G, s.chunk_bytes, ws.G, ws.chunk_bytes);
  CHECK(g.G >= 1 && g.chunk_bytes >= 64 && g.chunk_bytes <= kChunkMax && g.G <= g.chunk_bytes && (rows < 1 || g.G <= rows), "%lld rows a group, %lld bytes a chunk",
        g.G, g.chunk_bytes);
}

int main() {
  std::mt19937_64 rng(20261021);
  auto upto = [&](unsigned long long hi) { return (long long)(rng() % (hi + 1)); };
  // a magnitude first, then a value below it: small numbers come as often as large ones
  auto any = [&](int bits) { return upto((1ull << (1 + rng() % (unsigned)bits)) - 1); };
  for (int round = 0; round < 200000; ++round) {
    const size_t free_b = (size_t)any(40);                                  // up to 1 TiB; a quarter of it often below 1 MiB
    const long long G = round & 1 ? 0 : any(34), chunk = round & 2 ? 0 : any(34);
    check_one(free_b, G, chunk, any(36), any(36), any(33), 1 + any(20));
  }
  // the borders, crossed with each other
  const size_t frees[] = {0, 3, 4, (4u << 20) - 1, 4u << 20, (4u << 20) + 4, (16u << 20) - 1, 16u << 20, (32u << 20) - 1, 32u << 20, (size_t)1 << 32, ((size_t)1 << 34) - 1,
                          (size_t)1 << 34, ((size_t)1 << 35) - 1, (size_t)1 << 35, (size_t)288 << 30};
  const long long asks[] = {0, 1, 2, 63, 64, 65, 1 << 20, (1ll << 30) - 1, 1ll << 30, (1ll << 30) + 1, 1ll << 33};
  const long long texts[] = {0, 1, 62, 63, 64, 65, 1000, (1ll << 30) - 2, (1ll << 30) - 1, 1ll << 30, 1ll << 34};
  const long long bounds[] = {0, 1, 2, 63, 64, 65, 100000, 1ll << 31};
  const long long per_rows[] = {1, 8, 53, 8012, 1 << 20};
  for (size_t free_b : frees)
    for (long long G : asks)
      for (long long chunk : asks)
        for (long long text : texts)
          for (long long rows : bounds)
            for (long long per_row : per_rows) check_one(free_b, G, chunk, text, texts[(size_t)(rows + per_row) % 11], rows, per_row);
  printf("ok %lld\n", n_checks);
  return 0;
}
