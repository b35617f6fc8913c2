// The host arithmetic of the device table readers (tables_device.hip), free of any device call so that a plain C++ compiler
// builds it and tests/cpp/tables_plan_check.cpp can hold it to a model: which gzip members of a <species>.snps.gz hold a range of
// table rows, how many rows of each are in front of the range and how many inside it, which member carries the table's header
// line, and how the chosen members of all tables are cut into groups whose inflated text stays below a cap.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace midas {

// A gzip member as its header and trailer announce it: where its deflate data lies in the file, compressed and inflated bytes
// ('M','S' and ISIZE), table rows ('M','R').  A table's header line is a member of no rows in front of the others.
struct TableMemberSpan { uint64_t data; uint32_t clen, ulen; int64_t rows; };

// A member that holds rows of [row_begin, row_begin + n_rows): `skip` of its rows lie in front of the range, the `take` behind
// them are rows out_row ... of the range.  header: the member's first line is the table's header line, no row.
struct ChosenMember {
  int32_t table, member;
  int64_t skip, take, out_row;
  uint8_t header;
};

// The table's header line is the first line of its first member that holds any text (-1: no such member).
inline int32_t header_member(const TableMemberSpan* m, size_t n) {
  for (size_t k = 0; k < n; ++k)
    if (m[k].ulen != 0) return (int32_t)k;
  return -1;
}

// The members of one table that hold rows of the range, in file order, appended to `out`; returns the rows they add up to
// (n_rows, or fewer when the table ends inside the range).  Depends on nothing but the members and the range.
inline int64_t choose_members(const TableMemberSpan* m, size_t n, int32_t table, int64_t row_begin, int64_t n_rows, std::vector<ChosenMember>& out) {
  const int64_t row_end = row_begin + n_rows;
  const int32_t hdr = header_member(m, n);
  int64_t at = 0, taken = 0;
  for (size_t k = 0; k < n; ++k) {
    const int64_t lo = at, hi = at + m[k].rows;
    at = hi;
    const int64_t use_lo = lo > row_begin ? lo : row_begin, use_hi = hi < row_end ? hi : row_end;
    if (use_hi <= use_lo) continue;      // (no row of the member lies in the range: empty members and an empty range included)
    out.push_back(ChosenMember{table, (int32_t)k, use_lo - lo, use_hi - use_lo, use_lo - row_begin, (uint8_t)((int32_t)k == hdr ? 1 : 0)});
    taken += use_hi - use_lo;
  }
  return taken;
}

// Chosen members [lo, hi) go up and are inflated together: `text` bytes of inflated text, `comp` bytes of deflate data.
struct MemberGroup { size_t lo, hi; uint64_t text, comp; };

// Consecutive chosen members whose text stays at or below `cap` bytes; a member larger than the cap is a group by itself.
// Every member's text counts rounded up to 16 bytes: that is how the members lie in a group's text buffer.
inline uint64_t member_text_room(uint32_t ulen) { return ((uint64_t)ulen + 15u) & ~(uint64_t)15u; }
inline std::vector<MemberGroup> group_members(const std::vector<ChosenMember>& chosen, const std::vector<std::vector<TableMemberSpan>>& tables, uint64_t cap) {
  std::vector<MemberGroup> groups;
  for (size_t k = 0; k < chosen.size(); ++k) {
    const TableMemberSpan& m = tables[(size_t)chosen[k].table][(size_t)chosen[k].member];
    const uint64_t room = member_text_room(m.ulen);
    if (groups.empty() || groups.back().text + room > cap) groups.push_back(MemberGroup{k, k, 0, 0});
    MemberGroup& g = groups.back();
    g.hi = k + 1;
    g.text += room;
    g.comp += m.clen;
  }
  return groups;
}

}  // namespace midas
