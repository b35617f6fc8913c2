// The sizes of a walk over text matrices by row groups (RowGroups in sites_rows.h: two matrices; GeneRows in genes_rows.h: one),
// free of any device call so that a plain C++ compiler builds it and tests/cpp/row_group_plan_check.cpp can hold it to the
// formulas it replaced: the rows a group (G) and the bytes of every matrix's chunk, as the caller asks for them or, for a
// request of 0, from a quarter of the free device memory.
#pragma once
#include <algorithm>
#include <cstddef>

namespace midas {

constexpr long long kChunkMax = 1ll << 30;      // newline offsets are 32-bit

struct RowGroupPlan { long long G, chunk_bytes; };

// free_bytes: the free device memory; read only when group_rows or chunk_bytes is 0.  n_matrices chunks go up side by side.
// text_bytes: the largest matrix; n_rows_max: the rows the walk may read; per_row: the device bytes a row of the group takes.
// A chunk left to this function is a quarter of the budget over the matrices, at least 1 MiB; the groups get the budget less
// the chunks with their newline counts (5 / 4 of a chunk), at least half of it.  Then: a chunk holds 64 bytes to 1 GiB and no
// more than the largest matrix and its appended terminator; a group holds 1 row to n_rows_max, and no more rows than a chunk
// has bytes.
inline RowGroupPlan plan_row_groups(size_t free_bytes, long long group_rows, long long chunk_bytes, int n_matrices, long long text_bytes,
                                    long long n_rows_max, long long per_row) {
  long long G = group_rows, chunk = chunk_bytes;
  const long long budget = (long long)(free_bytes / 4);
  if (chunk == 0) chunk = std::min<long long>(kChunkMax, std::max<long long>(1 << 20, budget / (4 * n_matrices)));
  if (G == 0) G = std::max<long long>(1, (budget - std::min(budget / 2, 5 * chunk * n_matrices / 4)) / per_row);
  chunk = std::min(std::max<long long>(chunk, 64), kChunkMax);
  chunk = std::min(chunk, std::max<long long>(64, text_bytes + 1));
  G = std::max<long long>(1, std::min(std::min(G, n_rows_max), chunk));
  return RowGroupPlan{G, chunk};
}

}  // namespace midas
