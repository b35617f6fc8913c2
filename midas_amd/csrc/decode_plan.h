// The host arithmetic of the device BAM decode (bam_device.hip), free of any device call so that a plain C++ compiler builds it
// and tests/cpp/decode_plan_check.cpp can hold it to a model: where the regions of an inflate lie in its arena, how a streamed
// decode cuts a run of blocks into groups and how large a slot must be for the largest of them, and how the chunks of a record
// walk are stitched into one chain of records.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "hostio.h"

namespace midas {

inline size_t round256(size_t v) { return (v + 255) & ~(size_t)255; }

// Room for a stream's tokens and literals (bgzf_inflate.hip: a dword per match from the front, the literals from the end), in the
// 8-byte units InflateBlock counts it in.  First pass: as many bytes as the stream inflates to -- a BAM's block needs ~0.7 of that
// (8 000 tokens + 13 000 literals for 64 KiB) -- because device memory costs ~17 ms a gigabyte to allocate here and the match lists
// are the second largest buffer.  A stream that needs more says so (kInflateMatchRoom) and is decoded again with the bound's room:
// 4/3 of its bytes, a match per three bytes.
inline uint32_t first_pass_room(uint32_t ulen) { return ulen / 8u + 16u; }
inline uint32_t second_pass_room(uint32_t ulen) { return ulen / 3u + 1u; }

constexpr size_t kInflateBlockBytes = 40;       // sizeof(InflateBlock) (kernels.h; bam_device.hip asserts it)

// ONE allocation for everything an inflate needs: | inflated | compressed | blocks | status, match counts | crc | match lists |,
// every region rounded up to 256 bytes by itself.  Everything behind the inflated bytes is dead once the blocks are resolved: the
// decodes lay the walk's tables and their columns over it.
struct InflateLayout {
  size_t at_comp, at_blocks, at_status, at_crc, at_matches, end;
  InflateLayout(size_t inflated_bytes, size_t comp_bytes, size_t n_blocks, size_t match_room) {
    at_comp = round256(inflated_bytes + 64);
    at_blocks = at_comp + round256(comp_bytes + 512);
    at_status = at_blocks + round256(n_blocks * kInflateBlockBytes);
    at_crc = at_status + round256(n_blocks * 8);
    at_matches = at_crc + round256(n_blocks * 4);
    end = at_matches + round256(match_room * 8);
  }
};

// ---- the groups of a streamed decode -------------------------------------------------------------------------------------------
// A group is blocks [b_lo, b_hi) plus the `tail` blocks kept behind them for the record that straddles its end: [b_lo, b_ext) is
// what goes up and is inflated (comp / infl bytes, `room` units of first-pass match lists), into a slot whose offsets start at the
// group's first inflated byte u_lo; it wants the records that start below `stop`.
struct DecodeGroup {
  size_t b_lo, b_hi, b_ext;
  uint64_t u_lo, stop;
  size_t comp, infl, room;
  size_t n_blocks() const { return b_ext - b_lo; }
  InflateLayout layout() const { return InflateLayout(infl, comp, n_blocks(), room); }
};
struct StreamPlan {
  std::vector<DecodeGroup> groups;
  size_t slot_bytes = 0;        // a slot holds any of the groups
  uint64_t seg_stop = 0;        // the segment's stop, or its blocks' end if that comes first
  int64_t bad_block = -1;       // >= 0: this block lies in front of its group's first byte (no plan)
};
inline StreamPlan plan_groups(const InflateJob* jobs, size_t j_lo, size_t j_hi, size_t group_blocks, size_t tail, int32_t n_ref, uint64_t stop) {
  StreamPlan plan;
  const uint64_t seg_limit = jobs[j_hi - 1].upos + jobs[j_hi - 1].ulen;
  plan.seg_stop = stop < seg_limit ? stop : seg_limit;
  plan.groups.resize((j_hi - j_lo + group_blocks - 1) / group_blocks);
  for (size_t g = 0; g < plan.groups.size(); ++g) {
    DecodeGroup& G = plan.groups[g];
    G.b_lo = j_lo + g * group_blocks;
    G.b_hi = std::min(j_hi, G.b_lo + group_blocks);
    G.b_ext = std::min(j_hi, G.b_hi + tail);
    G.u_lo = jobs[G.b_lo].upos;
    G.stop = G.b_hi == j_hi ? plan.seg_stop : std::min<uint64_t>(plan.seg_stop, jobs[G.b_hi].upos);
    G.comp = (size_t)(jobs[G.b_ext - 1].cpos + jobs[G.b_ext - 1].clen + 8 - jobs[G.b_lo].cpos);
    G.infl = (size_t)(jobs[G.b_ext - 1].upos + jobs[G.b_ext - 1].ulen - G.u_lo);
    G.room = 0;
    for (size_t j = G.b_lo; j < G.b_ext; ++j) {
      if (jobs[j].cpos < jobs[G.b_lo].cpos || jobs[j].upos < G.u_lo) { plan.bad_block = (int64_t)j; return plan; }
      G.room += first_pass_room(jobs[j].ulen);
    }
    // (behind the inflated bytes: the dead compressed bytes, tables and match lists hold the walk's tables and the record offsets --
    // 8 bytes a record of >= 36: a quarter of the inflated bytes at most)
    const InflateLayout L = G.layout();
    const size_t walk_scratch = G.infl / 3 + ((size_t)4 << 20) + round256((size_t)(n_ref > 0 ? n_ref : 1) * 8);
    plan.slot_bytes = std::max(plan.slot_bytes, std::max(L.end + 256, L.at_comp + walk_scratch));
  }
  return plan;
}

// ---- the record walk's chunks and their stitching --------------------------------------------------------------------------------
// The host's side of a walk (kernels.h BamWalkParams): per chunk of at most 32 KiB what the walk is given (lo, hi, stop, limit,
// forced, start) and what it found (start, end, kept, unmapped, first_unmapped, bad); base: records in front of the chunk.
constexpr unsigned long long kWalkChunk = 32768ull;
constexpr unsigned long long kNoOffset = ~0ull;
struct ChunkWalk {
  std::vector<unsigned long long> lo, hi, stop, limit, start, end, first_unmapped, base;
  std::vector<uint8_t> forced;
  std::vector<uint32_t> kept, unmapped, bad;
  size_t size() const { return lo.size(); }
  // the chunks over [from, stop) of a segment that ends at `limit`; the first one starts at `from` exactly, or guesses like the rest
  void add_segment(unsigned long long from, unsigned long long seg_stop, unsigned long long seg_limit, bool exact) {
    for (unsigned long long at = from; at < seg_stop; at += kWalkChunk) {
      lo.push_back(at); hi.push_back(at + kWalkChunk < seg_stop ? at + kWalkChunk : seg_stop); stop.push_back(seg_stop); limit.push_back(seg_limit);
      const bool first = at == from;
      forced.push_back(first && exact ? 1 : 0);
      start.push_back(first && exact ? from : kNoOffset);
    }
  }
  void room_for_results() {       // (one entry at least: the device's tables are never empty)
    const size_t n = std::max<size_t>(size(), 1);
    end.resize(n); first_unmapped.resize(n); base.resize(n); kept.resize(n); unmapped.resize(n); bad.resize(n);
  }
  unsigned long long count_records() {      // base[c] = records of the chunks in front of c; all of them
    unsigned long long n = 0;
    for (size_t c = 0; c < size(); ++c) { base[c] = n; n += kept[c]; }
    return n;
  }
};

// One segment's chunks [c_lo, c_hi) stitched in order: a chunk belongs to the chain when its walk started where the chain stands;
// one whose guess the chain does not hit is walked again from there (`again(c, cur)`: start[c] = cur and the chunk's results anew;
// false: it could not, the caller knows why).  cur: where the chain starts, kNoOffset: at the first boundary a chunk guessed.
// Chunks in which no record of the chain starts are emptied (kept = unmapped = 0, start = none).  *rounds counts the second walks
// of all the segments of a decode: more than kStitchRounds of them and the boundaries are said not to settle.
constexpr int kStitchRounds = 4096;
enum class Stitch { settled, bad_chunk, unsettled, failed };
struct StitchResult {
  Stitch what = Stitch::settled;
  unsigned long long first = kNoOffset;            // the chain's first record (none: no chunk found a boundary)
  unsigned long long end = kNoOffset;              // where the chain ended: the first record start at or behind the stop (none: as `first`)
  unsigned long long first_unmapped = kNoOffset;
  long long n_records = 0, n_unmapped = 0;
};
template <class Again>
StitchResult stitch_chunks(ChunkWalk& w, size_t c_lo, size_t c_hi, unsigned long long cur, int* rounds, Again&& again) {
  StitchResult r;
  for (size_t c = c_lo; c < c_hi;) {
    if (cur == kNoOffset) {            // (a guessed first record: the first chunk that found a boundary gives it)
      if (w.start[c] == kNoOffset) { w.kept[c] = 0u; w.unmapped[c] = 0u; ++c; continue; }
      cur = w.start[c];
    }
    if (cur >= w.hi[c] || cur + 4 > w.limit[c]) { w.kept[c] = 0u; w.unmapped[c] = 0u; w.start[c] = kNoOffset; ++c; continue; }   // no record starts in this chunk
    if (w.start[c] == cur) {
      if (w.bad[c]) { r.what = Stitch::bad_chunk; return r; }
      if (r.first == kNoOffset) r.first = cur;
      r.n_records += w.kept[c];
      if (w.unmapped[c] && r.first_unmapped == kNoOffset) r.first_unmapped = w.first_unmapped[c];
      r.n_unmapped += w.unmapped[c];
      cur = w.end[c];
      ++c;
      continue;
    }
    if (++*rounds > kStitchRounds) { r.what = Stitch::unsettled; return r; }
    if (!again(c, cur)) { r.what = Stitch::failed; return r; }
  }
  r.end = cur;
  return r;
}

}  // namespace midas
