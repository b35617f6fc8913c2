// The host arithmetic of the device table readers (midas_amd/csrc/tables_plan.h) held to a row-by-row model: the members chosen for
// a row range, their skip / take counts, the header member, and the groups.  Stand-alone: prints "ok <checks>" and returns 0, or
// says what failed and returns 1.
#include "tables_plan.h"

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

// the model: every row of the table knows its member; the range picks rows one by one
struct ModelMember { int32_t member; int64_t first_in_member, rows_taken, first_out; };
static std::vector<ModelMember> model_choose(const std::vector<TableMemberSpan>& t, int64_t row_begin, int64_t n_rows) {
  std::vector<int32_t> member_of;
  std::vector<int64_t> index_in;
  for (size_t k = 0; k < t.size(); ++k)
    for (int64_t r = 0; r < t[k].rows; ++r) { member_of.push_back((int32_t)k); index_in.push_back(r); }
  std::vector<ModelMember> out;
  for (int64_t r = row_begin; r < row_begin + n_rows && r < (int64_t)member_of.size(); ++r) {
    if (out.empty() || out.back().member != member_of[(size_t)r]) out.push_back(ModelMember{member_of[(size_t)r], index_in[(size_t)r], 0, r - row_begin});
    ++out.back().rows_taken;
  }
  return out;
}

static std::vector<TableMemberSpan> random_table(std::mt19937& rng, int shape) {
  std::vector<TableMemberSpan> t;
  uint64_t at = 0;
  auto add = [&](uint32_t ulen, int64_t rows) {
    const uint32_t clen = ulen ? 2u + rng() % (ulen + 7u) : 2u;
    t.push_back(TableMemberSpan{at + 28, clen, ulen, rows});
    at += 28 + clen + 8;
  };
  if (shape & 1) add(0, 0);                        // an empty member in front of the header
  if (shape & 2) add(66, 0);                       // the header line in a member of its own
  const int n = (int)(rng() % 9);
  for (int k = 0; k < n; ++k) {
    const int kind = (int)(rng() % 8);
    if (kind == 0) add(0, 0);                      // an empty member among the others
    else if (kind == 1) add(1u + rng() % 40u, 1);
    else { const int64_t rows = 1 + (int64_t)(rng() % 40); add((uint32_t)rows * (20u + rng() % 30u), rows); }
  }
  return t;
}

static void check_one(std::mt19937& rng, int shape) {
  const int n_tables = 1 + (int)(rng() % 4);
  std::vector<std::vector<TableMemberSpan>> tables;
  for (int t = 0; t < n_tables; ++t) tables.push_back(random_table(rng, shape));
  int64_t longest = 0;
  for (const auto& t : tables) { int64_t r = 0; for (const auto& m : t) r += m.rows; if (r > longest) longest = r; }
  // ranges: anywhere, inside one member, empty, beyond the end
  const int64_t row_begin = (int64_t)(rng() % (uint32_t)(longest + 3));
  const int kind = (int)(rng() % 4);
  const int64_t n_rows = kind == 0 ? 0 : kind == 1 ? 1 + (int64_t)(rng() % 3) : (int64_t)(rng() % (uint32_t)(longest + 5));
  std::vector<ChosenMember> chosen;
  for (int t = 0; t < n_tables; ++t) {
    const size_t first = chosen.size();
    const int64_t taken = choose_members(tables[(size_t)t].data(), tables[(size_t)t].size(), t, row_begin, n_rows, chosen);
    const std::vector<ModelMember> want = model_choose(tables[(size_t)t], row_begin, n_rows);
    CHECK(chosen.size() - first == want.size(), "table %d rows [%lld, +%lld): %zu members chosen, the model has %zu", t, (long long)row_begin,
          (long long)n_rows, chosen.size() - first, want.size());
    int64_t sum = 0;
    const int32_t hdr = header_member(tables[(size_t)t].data(), tables[(size_t)t].size());
    CHECK(hdr < 0 || tables[(size_t)t][(size_t)hdr].ulen != 0, "header member %d of table %d is empty", hdr, t);
    for (int32_t k = 0; k < hdr; ++k) CHECK(tables[(size_t)t][(size_t)k].ulen == 0, "member %d in front of header member %d holds text", k, hdr);
    for (size_t k = 0; k < want.size(); ++k) {
      const ChosenMember& c = chosen[first + k];
      CHECK(c.table == t && c.member == want[k].member, "table %d: member %d chosen, the model has %d", t, c.member, want[k].member);
      CHECK(c.skip == want[k].first_in_member && c.take == want[k].rows_taken && c.out_row == want[k].first_out,
            "table %d member %d: skip %lld take %lld out_row %lld, the model has %lld %lld %lld", t, c.member, (long long)c.skip, (long long)c.take,
            (long long)c.out_row, (long long)want[k].first_in_member, (long long)want[k].rows_taken, (long long)want[k].first_out);
      CHECK(c.take > 0 && c.skip >= 0 && c.skip + c.take <= tables[(size_t)t][(size_t)c.member].rows, "table %d member %d: rows [%lld, +%lld) of %lld", t,
            c.member, (long long)c.skip, (long long)c.take, (long long)tables[(size_t)t][(size_t)c.member].rows);
      CHECK((c.header != 0) == (c.member == hdr), "table %d member %d: header %d, the header member is %d", t, c.member, (int)c.header, hdr);
      CHECK(c.out_row == sum, "table %d member %d lands at row %lld behind %lld rows", t, c.member, (long long)c.out_row, (long long)sum);
      sum += c.take;
    }
    int64_t rows = 0;
    for (const auto& m : tables[(size_t)t]) rows += m.rows;
    const int64_t in_range = row_begin >= rows ? 0 : (rows - row_begin < n_rows ? rows - row_begin : n_rows);
    CHECK(sum == taken && sum == in_range, "table %d: %lld rows taken (%lld returned), %lld of the range lie in the table", t, (long long)sum, (long long)taken,
          (long long)in_range);
  }
  // groups under several caps: the chosen members are the same whatever the cap (they were chosen without it)
  const uint64_t caps[5] = {1, 64, 1000, 65536, ~0ull};
  for (uint64_t cap : caps) {
    const std::vector<MemberGroup> groups = group_members(chosen, tables, cap);
    size_t at = 0;
    for (const MemberGroup& g : groups) {
      CHECK(g.lo == at && g.hi > g.lo && g.hi <= chosen.size(), "cap %llu: group [%zu, %zu) behind member %zu of %zu", (unsigned long long)cap, g.lo, g.hi, at,
            chosen.size());
      uint64_t text = 0, comp = 0;
      for (size_t k = g.lo; k < g.hi; ++k) {
        const TableMemberSpan& m = tables[(size_t)chosen[k].table][(size_t)chosen[k].member];
        text += (m.ulen + 15ull) / 16ull * 16ull;
        comp += m.clen;
      }
      CHECK(text == g.text && comp == g.comp, "cap %llu: group [%zu, %zu) says %llu + %llu bytes, its members hold %llu + %llu", (unsigned long long)cap, g.lo,
            g.hi, (unsigned long long)g.text, (unsigned long long)g.comp, (unsigned long long)text, (unsigned long long)comp);
      CHECK(text <= cap || g.hi - g.lo == 1, "cap %llu: group [%zu, %zu) holds %llu bytes of text", (unsigned long long)cap, g.lo, g.hi, (unsigned long long)text);
      if (g.hi < chosen.size()) {      // (greedy: the next member would not have fitted)
        const TableMemberSpan& nx = tables[(size_t)chosen[g.hi].table][(size_t)chosen[g.hi].member];
        CHECK(text + (nx.ulen + 15ull) / 16ull * 16ull > cap, "cap %llu: group [%zu, %zu) stops though member %zu fits", (unsigned long long)cap, g.lo, g.hi, g.hi);
      }
      at = g.hi;
    }
    CHECK(at == chosen.size(), "cap %llu: the groups end at member %zu of %zu", (unsigned long long)cap, at, chosen.size());
    if (cap == ~0ull) CHECK(groups.size() <= 1, "no cap: %zu groups", groups.size());
  }
}

int main() {
  std::mt19937 rng(20240917);
  for (int round = 0; round < 4000; ++round) check_one(rng, round & 3);
  // a header-only table, and a range inside one member
  {
    std::vector<TableMemberSpan> t = {{28, 40, 66, 0}};
    std::vector<ChosenMember> c;
    CHECK(choose_members(t.data(), t.size(), 0, 0, 10, c) == 0 && c.empty(), "a header-only table gave %zu members", c.size());
    CHECK(header_member(t.data(), t.size()) == 0, "header member of a header-only table");
    t.push_back({200, 500, 4000, 100});
    CHECK(choose_members(t.data(), t.size(), 0, 40, 5, c) == 5 && c.size() == 1 && c[0].member == 1 && c[0].skip == 40 && c[0].take == 5 && c[0].out_row == 0 &&
              c[0].header == 0, "a range inside one member");
  }
  printf("ok %lld\n", n_checks);
  return 0;
}
