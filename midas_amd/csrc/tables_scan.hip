// The rows of <species>.snps.gz members parsed on the device, where bgzf_inflate.hip left their text: the last four tab-separated
// fields of every row (count_a, count_c, count_g, count_t: r[-4:] of midas/merge/snps.py:262-270) as one 16-byte store into
// counts[row][4] -- the layout merge_sites.hip reads.  What midas_snps_tableset_read_counts does on the host's threads.
//
// A GROUP of members lies in one text buffer, every member at a multiple of 16 bytes.  The line index is built the way
// sites_rows.h and sam_scan.hip build theirs: line ends counted per 16-byte load, the library's exclusive scan, every end to its
// place.  Two things differ from a plain newline index, both because a member is a text of its own:
//   * a word belongs to ONE member (found by bisection over the members' starts) and only its bytes below the member's ISIZE
//     count: what lies between a member's end and the next member's start is never interpreted;
//   * a member's last byte ends a line whether it is a newline or not (parse_rows of tables_host.cpp accepts a last row
//     without one): its end is the member's end then.
// The lines of a member are consecutive in the index, so member m's line j is entry word_lines[start / 16] + j.
//
// ACCEPTED ROWS AND VALUES are parse_rows' (tables_host.cpp), the yardstick: at least 7 tabs; only the first 16 tabs of a row are
// noted, the four fields are the ones behind the last four NOTED tabs and the fourth runs to the end of the line -- a row of more
// than 16 tabs therefore offers fields 13-16 with the rest of the line in the fourth, and fails on the tab in it; every field
// non-empty, digits only, value <= 0x7FFFFFFF.  One thread per taken row; a malformed row lowers bad[table] to its table row.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "text_rows.h"

namespace midas {
namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// the member that owns word w: the last one that starts at or in front of it (members without text share their start with the
// next one and are never the last such), or -1 when the word lies behind that member's bytes
__device__ __forceinline__ int member_of_word(const TableTextMember* m, int n, long long w) {
  int lo = 0, hi = n;                   // the first member that starts behind w
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if ((long long)(m[mid].start >> 4) <= w) lo = mid + 1; else hi = mid;
  }
  const int k = lo - 1;
  if (k < 0) return -1;
  const unsigned long long end = (unsigned long long)m[k].start + m[k].ulen;
  return (unsigned long long)w * 16ull < end ? k : -1;
}

// What a word holds of its member: the newline flags of its valid bytes (bit 7 of every byte, per dword), and whether the
// member's last byte lies in it and is no newline (a line ends there all the same).
struct WordLines { uint32_t nl[4]; bool open_end; uint32_t end_pos; };
__device__ __forceinline__ WordLines word_lines_of(const TablesScanParams& p, const TableTextMember& mb, long long w) {
  WordLines r;
  const uint4 v = reinterpret_cast<const uint4*>(p.text)[w];
  const uint32_t d[4] = {v.x, v.y, v.z, v.w};
  const unsigned long long base = (unsigned long long)w * 16ull, end = (unsigned long long)mb.start + mb.ulen;
  const uint32_t valid = end - base < 16ull ? (uint32_t)(end - base) : 16u;       // 1..16: bytes of the word below the member's ISIZE
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const uint32_t nb = valid > 4u * (uint32_t)q ? (valid - 4u * (uint32_t)q < 4u ? valid - 4u * (uint32_t)q : 4u) : 0u;
    const uint32_t mask = nb >= 4u ? 0xFFFFFFFFu : ((1u << (8u * nb)) - 1u);
    r.nl[q] = newline_bytes(d[q]) & mask;
  }
  const bool last_here = end - base <= 16ull;
  const uint32_t lb = valid - 1u;
  const uint32_t last_byte = (d[lb >> 2] >> (8u * (lb & 3u))) & 255u;
  r.open_end = last_here && last_byte != (uint32_t)'\n';
  r.end_pos = (uint32_t)end;
  return r;
}

__global__ __launch_bounds__(256) void tables_count_kernel(TablesScanParams p) {
  const long long w = (long long)blockIdx.x * 256 + threadIdx.x;
  if (w > p.n16) return;
  uint32_t n = 0;
  if (w < p.n16) {
    const int k = member_of_word(p.members, p.n_members, w);
    if (k >= 0) {
      const WordLines wl = word_lines_of(p, p.members[k], w);
      n = __popc(wl.nl[0]) + __popc(wl.nl[1]) + __popc(wl.nl[2]) + __popc(wl.nl[3]) + (wl.open_end ? 1u : 0u);
    }
  }
  p.word_lines[w] = n;              // (entry n16: nothing, so that the scan leaves the number of all lines there)
}

__global__ __launch_bounds__(256) void tables_ends_kernel(TablesScanParams p) {
  const long long w = (long long)blockIdx.x * 256 + threadIdx.x;
  if (w >= p.n16) return;
  const int k = member_of_word(p.members, p.n_members, w);
  if (k < 0) return;
  const WordLines wl = word_lines_of(p, p.members[k], w);
  uint32_t at = p.word_lines[w];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    uint32_t m = wl.nl[q];
    while (m) {
      const int b = __ffs(m) - 1;          // bit 7, 15, 23 or 31
      if (at < p.cap_lines) p.line_end[at] = (uint32_t)(16 * w + 4 * q + (b >> 3));
      ++at;
      m &= m - 1;
    }
  }
  if (wl.open_end && at < p.cap_lines) p.line_end[at] = wl.end_pos;
}

// lines found in every member: the scan's values at its first word and behind its last
__global__ __launch_bounds__(256) void tables_member_lines_kernel(TablesScanParams p) {
  const int k = (int)(blockIdx.x * 256 + threadIdx.x);
  if (k >= p.n_members) return;
  const TableTextMember mb = p.members[k];
  const long long w0 = (long long)(mb.start >> 4), w1 = w0 + (((long long)mb.ulen + 15) >> 4);
  p.member_lines[k] = w1 <= p.n16 ? p.word_lines[w1] - p.word_lines[w0] : 0u;
}

__global__ __launch_bounds__(256) void tables_parse_kernel(TablesScanParams p) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= p.n_take) return;
  int lo = 0, hi = p.n_members;         // the last member whose taken rows start at or in front of row i
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if ((long long)p.members[mid].take_base <= i) lo = mid + 1; else hi = mid;
  }
  if (lo == 0) return;
  const TableTextMember mb = p.members[lo - 1];
  const uint32_t r = (uint32_t)(i - (long long)mb.take_base);
  if (r >= mb.take) return;
  const uint32_t head = mb.header ? 1u : 0u;
  if (p.member_lines[lo - 1] != head + mb.rows) return;       // (another number of rows than announced: the host says so)
  const uint32_t j = mb.skip + r;                             // the row within the member
  const uint32_t first = p.word_lines[mb.start >> 4];
  const uint32_t line = first + head + j;
  if (line >= p.cap_lines) return;
  const uint32_t member_end = mb.start + mb.ulen;
  uint32_t e = p.line_end[line];
  uint32_t b = line == first ? mb.start : p.line_end[line - 1u] + 1u;
  // (what the index says lies inside the member; held to it all the same: every byte read below is in [start, start + ulen))
  if (e > member_end) e = member_end;
  if (b < mb.start) b = mb.start;
  if (b > e) b = e;
  const uint8_t* t = p.text;
  // the first 16 tabs of the row, the last four of them kept (parse_rows: `tabs[16]`, fields behind tabs[nt - 4 .. nt - 1])
  uint32_t nt = 0, t0 = 0, t1 = 0, t2 = 0, t3 = 0;
  for (uint32_t q = b; q < e && nt < 16u; ++q) {
    if (t[q] == (uint8_t)'\t') { t0 = t1; t1 = t2; t2 = t3; t3 = q; ++nt; }
  }
  bool ok = nt >= 7u;
  const uint32_t fs[4] = {t0 + 1u, t1 + 1u, t2 + 1u, t3 + 1u}, fe[4] = {t1, t2, t3, e};
  uint32_t v4[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (ok) {
      unsigned long long v = 0;
      if (fs[k] >= fe[k]) ok = false;
      for (uint32_t q = fs[k]; q < fe[k] && ok; ++q) {
        const uint32_t c = t[q];
        if (c < (uint32_t)'0' || c > (uint32_t)'9') { ok = false; break; }
        v = v * 10ull + (c - (uint32_t)'0');
        if (v > 0x7FFFFFFFull) ok = false;       // major + minor of one sample must fit 32 bits downstream
      }
      v4[k] = (uint32_t)v;
    }
  }
  if (!ok) {
    atomicMin(&p.bad[mb.table], mb.table_row + j);
    return;
  }
  u32x4 out;
  out.x = v4[0]; out.y = v4[1]; out.z = v4[2]; out.w = v4[3];
  reinterpret_cast<u32x4*>(p.counts)[mb.dst_row + r] = out;
}

}  // namespace

hipError_t launch_tables_index(const TablesScanParams& p, hipStream_t s) {
  if (p.n_members <= 0) return hipSuccess;
  hipLaunchKernelGGL(tables_count_kernel, dim3(nblocks(p.n16 + 1, 256)), dim3(256), 0, s, p);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  e = launch_scan_u32(p.word_lines, p.word_lines, p.n16 + 1, p.scan_scratch, s);
  if (e != hipSuccess) return e;
  if (p.n16 > 0) hipLaunchKernelGGL(tables_ends_kernel, dim3(nblocks(p.n16, 256)), dim3(256), 0, s, p);
  hipLaunchKernelGGL(tables_member_lines_kernel, dim3(nblocks(p.n_members, 256)), dim3(256), 0, s, p);
  return hipGetLastError();
}

hipError_t launch_tables_parse(const TablesScanParams& p, hipStream_t s) {
  if (p.n_take <= 0 || p.n_members <= 0) return hipSuccess;
  hipLaunchKernelGGL(tables_parse_kernel, dim3(nblocks(p.n_take, 256)), dim3(256), 0, s, p);
  return hipGetLastError();
}

}  // namespace midas
